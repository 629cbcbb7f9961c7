"""HBM-resident graphs (``device_graph``), their row-sharded form and feature shards."""
from __future__ import annotations

__all__ = ["edge_list_factory"]

_EDGE_LIST_KEYS = ("src", "dst", "weight", "edge_type", "node_ids", "features", "labels")


def edge_list_factory(path_or_arrays, **from_edges_kwargs):
    """A ``params["device_graph_factory"]`` for an edge list: a callable ``(rank, device) ->
    DeviceGraph`` that builds the graph with :meth:`DeviceGraph.from_edges` on the rank's
    device, no graph engine involved.

    ``path_or_arrays``: an ``.npz`` file with the arrays ``src``, ``dst`` and, optionally,
    ``weight``, ``edge_type``, ``node_ids``, ``features``, ``labels`` -- or a dict of arrays
    under the same names.  ``from_edges_kwargs`` go to ``from_edges`` (``num_nodes``,
    ``symmetric``, ``duplicates``, ``feature_dtype``, ...)."""
    import os

    import numpy as np

    if isinstance(path_or_arrays, (str, os.PathLike)):
        with np.load(os.fspath(path_or_arrays), allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
    else:
        arrays = dict(path_or_arrays)
    unknown = sorted(set(arrays) - set(_EDGE_LIST_KEYS))
    if unknown:
        raise ValueError(f"edge_list_factory: unknown arrays {unknown}; known: {list(_EDGE_LIST_KEYS)}")
    for k in ("src", "dst"):
        if k not in arrays:
            raise ValueError(f"edge_list_factory: the edge list has no '{k}' array")

    def factory(rank, device):
        from euler_amd.graph.device_graph import DeviceGraph

        kw = dict(from_edges_kwargs)
        kw.setdefault("seed", int(rank))
        return DeviceGraph.from_edges(device=device, **arrays, **kw)

    return factory
