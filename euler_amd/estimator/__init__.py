"""Estimators (reference ``euler_estimator/python/*.py``)."""
from __future__ import annotations

import logging
import time

import numpy as np
import torch
import torch.nn.functional as F

import euler_amd.ops.graph_api as ge
from euler_amd.estimator.base import BaseEstimator, id_file_batches, latest_checkpoint

log = logging.getLogger("euler_amd.estimator")

__all__ = ["BaseEstimator", "NodeEstimator", "EdgeEstimator", "GraphEstimator", "GaeEstimator", "SampleEstimator",
           "latest_checkpoint", "id_file_batches"]


def _shard(est):
    return (est.rank, est.world)


class NodeEstimator(BaseEstimator):
    """train: ``sample_node(batch_size, train_node_type)``; eval / infer: id file
    (reference node_estimator.py:26-51)."""

    def get_train_from_input(self, inputs, params):
        return ge.sample_node(inputs, params["train_node_type"])

    def train_input_fn(self):
        return self.params["batch_size"]

    def get_input_from_id_file(self):
        for b in id_file_batches(self.params["id_file"], self.params["batch_size"], int, _shard(self)):
            yield torch.tensor(b, dtype=torch.int64)

    def evaluate_input_fn(self):
        return self.get_input_from_id_file()

    def infer_input_fn(self):
        return self.get_input_from_id_file()


class GaeEstimator(NodeEstimator):
    """Same inputs as NodeEstimator (reference gae_estimator.py:26-51)."""


class EdgeEstimator(BaseEstimator):
    """train: ``sample_edge(batch_size, train_edge_type)`` -> [n, 3] (src, dst, type);
    eval / infer: "src dst type" lines; ``infer_type`` picks node_src / edge / node_dst
    embeddings (reference edge_estimator.py:27-72)."""

    def get_train_from_input(self, inputs, params):
        return ge.sample_edge(inputs, params["train_edge_type"])

    def train_input_fn(self):
        return self.params["batch_size"]

    def transfer_embedding(self, source, emb):
        t = self.params.get("infer_type", "node_src")
        source = torch.as_tensor(source)
        if t == "node_src":
            return source[:, 0], emb[0]
        if t == "edge":
            return source[:, :2], emb[1]
        if t == "node_dst":
            return source[:, 1], emb[2]
        raise ValueError("infer_type must be node_src/node_dst/edge.")

    def get_input_from_id_file(self):
        def parse(line):
            a = line.split()
            return [int(a[0]), int(a[1]), int(a[2])]

        for b in id_file_batches(self.params["id_file"], self.params["batch_size"], parse, _shard(self)):
            yield torch.tensor(b, dtype=torch.int64)

    def evaluate_input_fn(self):
        return self.get_input_from_id_file()

    def infer_input_fn(self):
        return self.get_input_from_id_file()

    def _known_triples(self, num_entities):
        """the filter of :meth:`rank_evaluate`: every edge of params["rank_filter_edge_types"]
        (absent / None: every edge of the graph; []: none, i.e. raw ranking)"""
        from euler_amd.models.kg_eval import KnownTriples
        from euler_amd.ops import base

        types = self.params.get("rank_filter_edge_types")
        if types is not None and len(types) == 0:
            return None
        eng = base.get_engine()
        ids = [-1] if types is None else [int(np.asarray(ge.get_edge_type_id(t)).reshape(-1)[0]) for t in types]
        src, dst, rel = [], [], []
        for et in ids:
            s, d, _, feat = eng.export_edges(et, "dense_id", 1)
            src.append(np.asarray(s).astype(np.int64))
            dst.append(np.asarray(d).astype(np.int64))
            rel.append(np.asarray(feat).reshape(-1).astype(np.int64))
        return KnownTriples(np.concatenate(src), np.concatenate(rel), np.concatenate(dst), num_entities,
                            device=self.device)

    @torch.no_grad()
    def rank_evaluate(self):
        """Link prediction over the id file's triples ("src dst type" lines, relation = the
        edge feature ``id``): every true head and tail ranked against all entities
        (models/kg_eval.py), filtered by the known triples of
        params["rank_filter_edge_types"].  Returns ``link_prediction``'s dict (mrr / mr /
        hit@k over both sides, per side under "head" / "tail", and n).  Other params:
        ``rank_ties`` (pessimistic | optimistic | mean), ``rank_batch``, ``rank_ks``.  With
        several ranks each one ranks its share of the id file and the sums are all-reduced
        before the division.  :meth:`evaluate` keeps returning the training metric."""
        from euler_amd.models import kg_eval
        from euler_amd.parallel import dp

        self.model.to(self.device)
        self.model.eval()
        self.restore(strict=False)
        batches = [b for b in self.get_input_from_id_file()]
        triples = torch.cat(batches, 0) if batches else torch.zeros(0, 3, dtype=torch.int64)
        src, dst = triples[:, 0], triples[:, 1]
        rel = torch.zeros(0, dtype=torch.int64)
        if triples.shape[0]:
            rel = torch.as_tensor(ge.get_edge_dense_feature(triples, ["id"], [1])[0]).reshape(-1).long()
        known = self._known_triples(int(self.model.node_max_id) + 1)
        ks = tuple(int(k) for k in self.params.get("rank_ks", (1, 3, 10)))
        t0 = time.time()
        ranks = kg_eval.rank_triples(self.model, src, rel, dst, known=known,
                                     ties=self.params.get("rank_ties", "pessimistic"),
                                     batch=int(self.params.get("rank_batch", 4096)))
        sums = torch.stack([kg_eval.rank_sums(ranks[s], ks) for s in ("head", "tail")])
        if dp.is_distributed():
            import torch.distributed as dist

            sums = sums if dist.get_backend() == "nccl" else sums.cpu()
            dist.all_reduce(sums)
        res = kg_eval.metrics_from_sums(sums.sum(0), ks)
        res["head"] = kg_eval.metrics_from_sums(sums[0], ks)
        res["tail"] = kg_eval.metrics_from_sums(sums[1], ks)
        res["n"] = int(sums[0, -1])
        if self.rank == 0:
            log.info("rank_evaluate (%s, %d triples, %.2f s): %s", "raw" if known is None else
                     "filtered by %d known triples" % len(known), res["n"], time.time() - t0,
                     {k: v for k, v in res.items() if not isinstance(v, dict)})
        return res


class GraphEstimator(BaseEstimator):
    """Graph classification: ``sample_graph_label`` -> ``get_graph_by_label`` ->
    {node_idx, graph_label (one-hot of the first node's label feature),
    node_graph_idx, graph_idx} (reference graph_estimator.py:27-85)."""

    def train_input_fn(self):
        return self.params["batch_size"]

    def get_graph_label(self, sample_graph):
        ind = torch.as_tensor(sample_graph.indices)
        vals = torch.as_tensor(sample_graph.values)
        first = vals[ind[:, 1] == 0]
        lab = ge.get_dense_feature(first, _as_list(self.params["label"]), [1])[0]
        lab = lab.reshape(-1).long()
        return F.one_hot(lab, int(self.params["num_classes"])).float()

    def _graph_inputs(self, labels):
        sg = ge.get_graph_by_label(labels)
        return {"node_idx": torch.as_tensor(sg.values), "graph_label": self.get_graph_label(sg),
                "node_graph_idx": torch.as_tensor(sg.indices)[:, 0], "graph_idx": labels}

    def get_train_from_input(self, inputs, params):
        return self._graph_inputs(ge.sample_graph_label(inputs))

    def get_input_from_id_file(self):
        for b in id_file_batches(self.params["id_file"], self.params["batch_size"], str, _shard(self)):
            yield b

    def get_evaluate_from_input(self, inputs, params):
        return self._graph_inputs(inputs)

    def get_infer_from_input(self, inputs, params):
        return self._graph_inputs(inputs)

    def transfer_embedding(self, source, emb):
        return np.asarray(source["graph_idx"]), emb

    def evaluate_input_fn(self):
        return self.get_input_from_id_file()

    def infer_input_fn(self):
        return self.get_input_from_id_file()


class SampleEstimator(BaseEstimator):
    """Explicit CSV sample rows, repeated ``epoch`` times for training
    (reference sample_estimator.py:25-53).  Each batch is a list of token lists."""

    def get_input_from_sample(self, epochs):
        for _ in range(int(epochs)):
            for b in id_file_batches(self.params["sample_dir"], self.params["batch_size"],
                                     lambda s: s.split(","), _shard(self)):
                yield b

    def train_input_fn(self):
        it = self.get_input_from_sample(self.params.get("epoch", 1))
        if self.params.get("total_step") is None:
            # one pass over the file defines the step count, like estimator.train(steps=None)
            batches = list(it)
            self.params["total_step"] = len(batches)
            it = iter(batches)
        return it

    def get_train_from_input(self, inputs, params):
        return next(inputs)

    def evaluate_input_fn(self):
        return self.get_input_from_sample(1)

    def infer_input_fn(self):
        return self.get_input_from_sample(1)

    def transfer_embedding(self, source, emb):
        # the target node is the second column of every row
        return np.asarray([int(r[1]) for r in source], dtype=np.int64).reshape(-1, 1), emb


def _as_list(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]
