"""Layer-wise full-neighbourhood inference for the GCN family on an HBM-resident graph.

``GcnTrainer.infer_logits`` builds an exact block per id batch and normalises with the
*in-block* source counts, so a node's embedding depends on its companions in the batch.
Layer-wise inference computes layer 0 for every node from all of its edges with the graph's
own degrees, keeps ``h0`` as a table, computes layer 1 from ``h0`` and so on: every layer
touches every edge once, and the result is deterministic and independent of the request.  With
every node a root of one block the two compute the same function.

Layer ``k`` of the model uses the mask of hop ``L - 1 - k`` and the scales
``(a_k, b_k) = gcn_scales(graph, mask, self_loops)`` (``ops/gcn_csr_ops.py``):
``h_k = relu((a_k * sum_e b_k[nbr_e] h_{k-1}[nbr_e]) @ W_k^T)``.  Layer 0 loads ``b_0`` per edge
of the raw feature table; every layer ``k < L - 1`` writes ``b_{k+1} * h_k`` (its ``out_scale``),
so the later layers read a table that already carries the source norm and load no scale per
edge.  FastGCN and AdaptiveGCN sample layers only to train: at inference they are this plain
GCN over their metapath.

``hidden()`` runs layers ``0 .. L - 2`` over all rows (in row chunks) into ``[N, Hp]`` tables and
caches the last one; ``embed(rows)`` / ``logits(rows)`` run the last conv layer for the requested
rows only, then ``fc`` (+ bias) and ``out_fc`` through ``gnn_ops.gemm``.

On the GPU the tables and conv weights are bf16 in the kernel's padded layout (table widths
to 16 columns, conv widths to 64) and every layer is one ``gcn_csr_fwd`` launch per row chunk;
on a CPU graph the same layers run as the fp32 composition.
"""
from __future__ import annotations

import torch

from euler_amd.ops import gnn_ops
from euler_amd.ops.gcn_csr_ops import gcn_csr_layer, gcn_scales

__all__ = ["LayerwiseGcnInference"]


def _up(n, m):
    return -(-int(n) // m) * m


def _padded(w, rows, cols, dtype):
    out = torch.zeros((rows, cols), dtype=dtype, device=w.device)
    out[: w.shape[0], : w.shape[1]] = w.detach()
    return out


class LayerwiseGcnInference:
    def __init__(self, graph, features, conv_weights, masks, self_loops, fc=None, out_fc=None, row_chunk=1 << 22,
                 embed_dim=None, logits_dim=None, impl=None):
        """``features`` [N, D0] (bf16 / fp32; on the GPU a width that is no multiple of 16 is
        padded once); ``conv_weights[k]`` [H_k, H_{k-1}] of model layer k in logical widths
        (H_{-1} = the feature width, or the padded table's); ``masks`` (edge-type bit sets) per
        hop, hop 0 next to the roots; ``fc`` = (weight [E, H_{L-1}], bias [E] or None) or None;
        ``out_fc`` = weight [C, E] or None.  ``embed_dim`` / ``logits_dim`` cut the outputs.
        ``impl``: "fused" (default on a GPU graph) or "composed" (default, and the only one,
        on a CPU graph)."""
        self.graph = graph
        self.device = graph.device
        self.on_gpu = self.device.type == "cuda"
        self.impl = impl or ("fused" if self.on_gpu else "composed")
        if self.impl == "fused" and not self.on_gpu:
            raise ValueError("impl='fused' needs a graph on the GPU")
        self.masks = [int(m) for m in masks]
        self.L = len(self.masks)
        if self.L < 1 or len(conv_weights) != self.L:
            raise ValueError("one conv weight and mask per hop")
        self.self_loops = bool(self_loops)
        if features.shape[0] != graph.num_rows:
            raise ValueError("features must have one row per graph row")
        if self.on_gpu and (features.shape[1] % 16 or not features.is_contiguous()):
            features = _padded(features, features.shape[0], _up(features.shape[1], 16), features.dtype)
        self.features = features
        self.row_chunk = max(64, int(row_chunk))
        self.embed_dim, self.logits_dim = embed_dim, logits_dim
        self.table_dtype = torch.bfloat16 if self.on_gpu else torch.float32
        # layer k's (a, b): the scales of hop L - 1 - k
        self.scales = [gcn_scales(graph, self.masks[self.L - 1 - k], self.self_loops) for k in range(self.L)]
        self.set_weights(conv_weights, fc, out_fc)

    # ------------------------------------------------------------------ parameters
    def set_weights(self, conv_weights, fc=None, out_fc=None):
        """new parameters (logical widths): the cached hidden table is dropped"""
        wdt = torch.bfloat16 if self.on_gpu else torch.float32
        width, convs = self.features.shape[1], []
        for k, w in enumerate(conv_weights):
            if w.dim() != 2 or w.shape[1] > width:
                raise ValueError(f"conv_weights[{k}] must be [H, <= {width}], got {tuple(w.shape)}")
            hp = _up(w.shape[0], 64) if self.on_gpu else w.shape[0]
            convs.append(_padded(w.to(self.device), hp, width, wdt))
            width = hp
        self.conv_weights = convs
        self.fc = None
        if fc is not None:
            w, b = fc
            self.fc = (_padded(w.to(self.device), w.shape[0], width, wdt),
                       None if b is None else b.detach().to(self.device).float().contiguous())
        self.out_fc = None if out_fc is None else out_fc.detach().to(self.device, wdt).contiguous()
        self.invalidate()

    def invalidate(self):
        self._hidden = None

    # ------------------------------------------------------------------ layers
    def _layer(self, k, x, rows, out=None):
        a, b = self.scales[k]
        return gcn_csr_layer(self.graph, x, self.conv_weights[k], mask=self.masks[self.L - 1 - k], rows=rows,
                             tgt_scale=a, src_scale=b if k == 0 else None,
                             out_scale=self.scales[k + 1][1] if k < self.L - 1 else None, self_loop=self.self_loops,
                             relu=True, out_dtype=self.table_dtype, impl=self.impl, out=out)

    @torch.no_grad()
    def hidden(self):
        """the input table of the last conv layer: the features for a 1-hop model, else
        ``b_{L-1} * h_{L-2}`` [N, H_{L-2}] of all rows (cached until the parameters change)"""
        if self.L == 1:
            return self.features
        if self._hidden is not None:
            return self._hidden
        N = self.graph.num_rows
        x = self.features
        for k in range(self.L - 1):
            out = torch.empty((N, self.conv_weights[k].shape[0]), dtype=self.table_dtype, device=self.device)
            for s in range(0, N, self.row_chunk):
                e = min(N, s + self.row_chunk)
                self._layer(k, x, range(s, e), out[s:e])
            x = out
        self._hidden = x
        return x

    @torch.no_grad()
    def last_conv(self, rows=None):
        """h_{L-1} of the requested rows (None: every row), in the table dtype"""
        if rows is not None:
            rows = torch.as_tensor(rows).to(self.device).reshape(-1)
        return self._layer(self.L - 1, self.hidden(), rows)

    @torch.no_grad()
    def embed(self, rows=None):
        """fp32 ``fc(h_{L-1})`` of the requested rows ([n, E]; h_{L-1} itself without fc)"""
        h = self.last_conv(rows)
        if self.fc is None:
            emb = h.float()
        else:
            emb = gnn_ops.gemm(h, self.fc[0], trans_b=True, bias=self.fc[1], out_dtype=torch.float32)
        return emb if self.embed_dim is None else emb[:, : self.embed_dim]

    @torch.no_grad()
    def logits(self, rows=None):
        """(embeddings [n, E], logits [n, C]) of the requested rows, fp32"""
        if self.out_fc is None:
            raise ValueError("logits() needs out_fc")
        emb = self.embed(rows)
        lg = gnn_ops.gemm(emb, self.out_fc, trans_b=True, out_dtype=torch.float32)
        return emb, lg if self.logits_dim is None else lg[:, : self.logits_dim]
