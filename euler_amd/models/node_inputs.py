"""Node inputs of the encoder models from the HBM graph: ``ShallowEncoder.forward``
(``utils/encoders.py``; reference ``tf_euler/python/utils/encoders.py:32-171``) over graph
*rows* instead of raw ids, for the device-path trainers.

The engine path reads sparse features on the host per batch and builds a data-dependent
SparseTensor; here the dense columns come from ``graph.features`` (``mp_ops.gather``), the
id embedding and every sparse-feature embedding bag from one fixed-shape kernel each
(``mp_ops.node_bag`` over ``graph.ids`` / ``graph.sparse``), so a whole step captures into
a hipGraph.  A negative row (the samplers' default node, the padding of a capacity-padded
hop set) reads zero dense features and the default id ``max_id + 1`` of every table, like
the engine's default node.
"""
from __future__ import annotations

import numpy as np
import torch

from euler_amd.ops import mp_ops

__all__ = ["DeviceNodeInputs", "MAX_TABLE_ROWS"]

MAX_TABLE_ROWS = 1 << 20  # estimator/device_trainers.py ROW_SPARSE_AUTO_ROWS


class DeviceNodeInputs:
    """``__call__(rows) -> [n, ne.output_dim]`` of a :class:`ShallowEncoder` ``ne`` on a
    :class:`~euler_amd.graph.device_graph.DeviceGraph`; the tables stay ``ne``'s own
    parameters (gradients flow to them through ``node_bag``)."""

    def __init__(self, ne, graph):
        from euler_amd.utils.layers import HashEmbedding, HashSparseEmbedding

        self.ne, self.graph = ne, graph
        self.features = graph.features if ne.use_feature else None
        if ne.use_feature and self.features is None:
            raise ValueError("the device graph needs the encoder's dense features (DeviceGraph.from_engine)")
        self.tables = []  # (layer, mode, hash, index) in ShallowEncoder.forward's order of the embeddings
        if ne.use_id:
            self._check_table(ne.embedding)
            self.tables.append((ne.embedding, "id", isinstance(ne.embedding, HashEmbedding), self._id_column(graph)))
        if ne.use_sparse_feature:
            for name, layer in zip(ne.sparse_feature_idx, ne.sparse_embeddings):
                if name not in graph.sparse:
                    raise ValueError("the device graph holds no sparse feature %r (DeviceGraph.from_engine("
                                     "sparse_features=...)); it has %s" % (name, sorted(graph.sparse)))
                self._check_table(layer)
                mode = "bag_mean" if layer.combiner == "mean" else "bag_sum"
                self.tables.append((layer, mode, isinstance(layer, HashSparseEmbedding), graph.sparse[name]))
        if not self.tables and not ne.use_feature:
            raise ValueError("the node encoder has no input (feature_idx, max_id and sparse_feature_idx are all unset)")

    @staticmethod
    def _check_table(layer):
        w = layer.weight
        if w.dtype != torch.float32:
            raise ValueError("device-path id / sparse-feature tables must be fp32 (got %s)" % w.dtype)
        if w.shape[0] >= MAX_TABLE_ROWS:
            raise ValueError("device-path id / sparse-feature tables are trained densely and take fewer than 2^20 rows "
                             "(got %d); larger tables need the row-sparse table path" % w.shape[0])

    @staticmethod
    def _id_column(graph):
        """raw node id of every row on the device, or None when row i is node i (a graph
        without an id column, e.g. ``DeviceGraph.synthetic``, or contiguous ids)"""
        if not hasattr(graph, "ids"):
            raise ValueError("use_id on the device path needs the graph's node ids (graph.ids)")
        if graph.ids is None:
            return None
        a = np.asarray(graph.ids, dtype=np.uint64).reshape(-1)
        if a.shape[0] and bool((a == np.arange(a.shape[0], dtype=np.uint64)).all()):
            return None
        return torch.from_numpy(a.view(np.int64).copy()).to(graph.device)

    def dense(self, rows):
        x = mp_ops.gather(self.features, rows.clamp(min=0)).float()
        return x * (rows >= 0).unsqueeze(1).to(x.dtype)  # the default node: zeros

    def __call__(self, rows):
        ne = self.ne
        rows = rows.reshape(-1).long()
        if not self.tables:  # dense columns only: the gather is the input
            x = self.dense(rows)
            return ne.dense(x) if ne.combiner == "add" or ne.dim else x
        if ne.combiner == "add":
            embs = [mp_ops.node_bag(layer.weight, rows, ix, mode, hsh) for layer, mode, hsh, ix in self.tables]
            if ne.use_feature:
                embs.insert(1 if ne.use_id else 0, ne.dense(self.dense(rows)))
            emb = embs[0]
            for e in embs[1:]:
                emb = emb + e
            return emb
        # concat: the embeddings land in their columns of one buffer (no torch.cat)
        widths = [layer.dim for layer, _, _, _ in self.tables]
        if ne.use_feature:
            widths.insert(1 if ne.use_id else 0, int(self.features.shape[1]))
        dev = self.features.device if self.features is not None else self.tables[0][0].weight.device
        out = torch.empty((rows.numel(), sum(widths)), dtype=torch.float32, device=dev)
        col, k = 0, 0
        for i, w in enumerate(widths):
            if ne.use_feature and i == (1 if ne.use_id else 0):
                out[:, col: col + w] = self.dense(rows)
            else:
                layer, mode, hsh, ix = self.tables[k]
                out = mp_ops.node_bag(layer.weight, rows, ix, mode, hsh, out=out, col=col)
                k += 1
            col += w
        return ne.dense(out) if ne.dim else out
