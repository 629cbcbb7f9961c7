"""Link prediction for the knowledge-graph models (``models/knowledge_graph.py``): rank the
true head or tail of every test triple against all entities, optionally without the other
known true answers (the "filtered" setting), and report MRR / MR / Hits@k.

* ``KnownTriples(src, rel, dst, num_entities)`` — the known triples, sorted by (rel, src)
  and by (rel, dst); gives the tail-side and head-side filter lists of a batch as CSRs.
* ``rank_triples(model, src, rel, dst, ...)`` — exact ranks per side.
* ``link_prediction(model, test, ...)`` — the metrics.

The hot loop, every query against every entity, is ``ops/kg_rank_ops.rank_counts``: on the
GPU a fused gfx950 kernel that never materialises a [queries, entities] score matrix, on the
CPU a chunked torch twin.  The model supplies its score in three parts (``entity_space``,
``relation_row``, ``rank_query`` and ``rank_kind``), computed with the class's own
normalisation / projection functions, so the ranking cannot drift from training.

Tie rule (``ties``): with ``better`` candidates scoring strictly better than the true entity
and ``ties`` scoring exactly the same, the rank is ``1 + better + ties`` ("pessimistic", the
rule of ``dataset.synthetic.tail_ranks``), ``1 + better`` ("optimistic") or
``1 + better + ties / 2`` ("mean": float64, the others int64).
"""
from __future__ import annotations

import torch

from euler_amd.ops import kg_rank_ops

__all__ = ["KnownTriples", "rank_triples", "rank_sums", "metrics_from_sums", "link_prediction", "TIE_RULES"]

TIE_RULES = ("pessimistic", "optimistic", "mean")
SIDES = ("head", "tail")


def _ids(t, device=None):
    t = torch.as_tensor(t).reshape(-1).long()
    return t if device is None else t.to(device)


class KnownTriples:
    """The set of known true triples, for filtered ranking.

    Kept twice, as sorted packed keys: by ``(rel, src)`` with the tails as values (the answers
    to (h, r, ?)) and by ``(rel, dst)`` with the heads as values (the answers to (?, r, t)).
    Repeated triples are stored once.  Values ascend inside a list, as ``rank_counts`` needs."""

    def __init__(self, src, rel, dst, num_entities, device=None):
        src, rel, dst = _ids(src, device), _ids(rel, device), _ids(dst, device)
        if not (src.numel() == rel.numel() == dst.numel()):
            raise ValueError("KnownTriples: src, rel and dst must have the same length")
        self.num_entities = n = int(num_entities)
        if src.numel() and (int(torch.min(torch.minimum(src, dst))) < 0 or int(torch.max(torch.maximum(src, dst))) >= n
                            or int(rel.min()) < 0):
            raise ValueError("KnownTriples: entity ids must be in [0, %d) and relation ids >= 0" % n)
        if src.numel() and (int(rel.max()) + 1) * n * n >= 2 ** 63:
            raise ValueError("KnownTriples: (relations * entities^2) = %d * %d^2 does not fit the packed int64 keys"
                             % (int(rel.max()) + 1, n))
        self.device = src.device
        self.tail_keys, self.tail_vals = self._index(rel * n + src, dst, n)
        self.head_keys, self.head_vals = self._index(rel * n + dst, src, n)

    @staticmethod
    def _index(keys, vals, n):
        packed = torch.unique(keys * n + vals)  # sorted: by key, then value; duplicates dropped
        return packed // n, (packed % n).to(torch.int32)

    def __len__(self):
        return int(self.tail_keys.numel())

    def to(self, device):
        """a copy on ``device`` (this object itself if it is there already), like Tensor.to"""
        device = torch.device(device)
        if device == self.device:
            return self
        other = object.__new__(KnownTriples)
        other.num_entities = self.num_entities
        for name in ("tail_keys", "tail_vals", "head_keys", "head_vals"):
            setattr(other, name, getattr(self, name).to(device))
        other.device = other.tail_keys.device
        return other

    def _csr(self, keys, vals, query):
        lo = torch.searchsorted(keys, query)
        hi = torch.searchsorted(keys, query, right=True)
        ln = hi - lo
        ptr = torch.zeros(query.numel() + 1, dtype=torch.long, device=query.device)
        ptr[1:] = ln.cumsum(0)
        total = int(ptr[-1])  # the one host read of a batch's filter
        off = torch.arange(total, device=query.device) - torch.repeat_interleave(ptr[:-1], ln, output_size=total)
        return ptr, vals[torch.repeat_interleave(lo, ln, output_size=total) + off]

    def tail_filter(self, src, rel):
        """(filt_ptr [B + 1] int64, filt_idx int32): the known tails of every (src, rel)"""
        src, rel = _ids(src, self.device), _ids(rel, self.device)
        return self._csr(self.tail_keys, self.tail_vals, rel * self.num_entities + src)

    def head_filter(self, dst, rel):
        """(filt_ptr [B + 1] int64, filt_idx int32): the known heads of every (rel, dst)"""
        dst, rel = _ids(dst, self.device), _ids(rel, self.device)
        return self._csr(self.head_keys, self.head_vals, rel * self.num_entities + dst)

    def filter(self, side, src, rel, dst):
        return self.tail_filter(src, rel) if side == "tail" else self.head_filter(dst, rel)


def _to_positions(ptr, idx, pos):
    """entity ids of a filter CSR -> positions in a candidate subset (``pos[id]``, -1: not a
    candidate, dropped); ``pos`` is monotone over the candidates, so the lists stay ascending"""
    p = pos[idx.long()]
    keep = p >= 0
    csum = torch.zeros(idx.numel() + 1, dtype=torch.long, device=idx.device)
    csum[1:] = keep.long().cumsum(0)
    return csum[ptr], p[keep].to(torch.int32)


def _ranks(better, ties, rule):
    if rule == "pessimistic":
        return 1 + better + ties
    if rule == "optimistic":
        return 1 + better
    return 1.0 + better.double() + ties.double() / 2


@torch.no_grad()
def rank_triples(model, src, rel, dst, known=None, sides=SIDES, ties="pessimistic", batch=4096, cands=None):
    """``{side: ranks [n]}`` of the test triples ``(src[i], rel[i], dst[i])`` under ``model``
    (a ``TransX``): side "tail" ranks ``dst`` among the answers to (src, rel, ?), side "head"
    ranks ``src`` among the answers to (?, rel, dst); rank 1 is best.

    ``known``: a ``KnownTriples``; its other true answers are taken out of the candidates
    (filtered setting; one that lives on another device is copied to the model's for the
    call, the caller's object is left as it is).  None: raw ranking.  ``ties``: see the module
    docstring.  ``batch``: queries per ``rank_counts`` call.  ``cands``: an id subset to rank
    among (it must contain every true entity), e.g. the hubs of a typed KG; default all
    entities 0..node_max_id.

    For relation-dependent models (TransH / TransR / TransD) the triples are grouped by
    relation and ``entity_space(r)`` is built once per relation."""
    if ties not in TIE_RULES:
        raise ValueError("ties must be one of %s, got %r" % (TIE_RULES, ties))
    sides = tuple(sides)
    for s in sides:
        if s not in SIDES:
            raise ValueError("sides must be 'head' / 'tail', got %r" % (s,))
    if getattr(model, "entity_encoder", None) is not None:
        model._rank_table()  # a row-sharded table raises here, before any work
    dev = model._dev()
    src, rel, dst = _ids(src, dev), _ids(rel, dev), _ids(dst, dev)
    n = src.numel()
    if not (rel.numel() == n and dst.numel() == n):
        raise ValueError("rank_triples: src, rel and dst must have the same length")
    num_ent = int(model.node_max_id) + 1
    out = {s: torch.zeros(n, dtype=torch.float64 if ties == "mean" else torch.long, device=dev) for s in sides}
    if n == 0:
        return out
    if int(torch.min(torch.minimum(src, dst))) < 0 or int(torch.max(torch.maximum(src, dst))) >= num_ent:
        raise ValueError("rank_triples: entity ids must be in [0, %d)" % num_ent)
    if known is not None:
        if known.num_entities != num_ent:
            raise ValueError("rank_triples: known has %d entities, the model %d" % (known.num_entities, num_ent))
        known = known.to(dev)  # a copy local to this call when it lives elsewhere
    pos = None
    if cands is not None:
        cands = torch.unique(_ids(cands, dev))  # ascending: positions are monotone in the id
        if cands.numel() == 0 or int(cands[0]) < 0 or int(cands[-1]) >= num_ent:
            raise ValueError("rank_triples: cands must be entity ids in [0, %d)" % num_ent)
        pos = torch.full((num_ent,), -1, dtype=torch.long, device=dev)
        pos[cands] = torch.arange(cands.numel(), device=dev)
        for s, true in (("tail", dst), ("head", src)):
            if s in sides and bool((pos[true] < 0).any()):
                raise ValueError("rank_triples: a true %s entity is not among cands" % s)
    kind = model.rank_kind
    batch = max(1, int(batch))

    def run(space, rho_of, sel):
        """rank the triples ``sel`` (indices) against the candidate rows of ``space``"""
        table = (space if cands is None else space[cands]).contiguous().float()
        for a in range(0, sel.numel(), batch):
            ix = sel[a:a + batch]
            h, r, t = src[ix], rel[ix], dst[ix]
            rho = rho_of(r)
            for s in sides:
                given, true = (h, t) if s == "tail" else (t, h)
                q = model.rank_query(space[given], rho, s).contiguous().float()
                ptr = idx = None
                if known is not None:
                    ptr, idx = known.filter(s, h, r, t)
                    if pos is not None:
                        ptr, idx = _to_positions(ptr, idx, pos)
                true_pos = true if pos is None else pos[true]
                better, tie = kg_rank_ops.rank_counts(q, table, true_pos.contiguous(), kind, ptr, idx)
                out[s][ix] = _ranks(better, tie, ties)

    if not model.relation_dependent:
        run(model.entity_space(), model.relation_row, torch.arange(n, device=dev))
    else:
        order = torch.argsort(rel, stable=True)
        rels, counts = torch.unique_consecutive(rel[order], return_counts=True)
        start = 0
        for r, c in zip(rels.tolist(), counts.tolist()):
            rho = model.relation_row(r)
            run(model.entity_space(r), lambda _r, rho=rho: rho, order[start:start + c])
            start += c
    return out


def rank_sums(ranks, ks=(1, 3, 10)):
    """float64 ``[sum 1 / rank, sum rank, hits@k ..., n]`` of a rank vector: the additive
    form of the metrics (what data-parallel ranks all-reduce before the division)"""
    r = ranks.double()
    parts = [(1.0 / r).sum(), r.sum()] + [(r <= k).double().sum() for k in ks]
    parts.append(torch.tensor(float(r.numel()), dtype=torch.float64, device=r.device))
    return torch.stack(parts)


def metrics_from_sums(sums, ks=(1, 3, 10)):
    s = [float(x) for x in sums]
    n = max(s[-1], 1.0)
    res = {"mrr": s[0] / n, "mr": s[1] / n}
    for i, k in enumerate(ks):
        res["hit@%d" % k] = s[2 + i] / n
    return res


def link_prediction(model, test, known=None, ks=(1, 3, 10), **kw):
    """MRR / MR / Hits@k of the test triples ``test = (src, rel, dst)`` under ``model``.

    Returns ``{"mrr", "mr", "hit@k" ...}`` over both sides (every ranked (triple, side) pair
    weighs the same), the same keys per side under ``"head"`` and ``"tail"``, and ``"n"``, the
    number of test triples.  Ranks are exact; the metrics are computed in float64.  Keyword
    arguments go to :func:`rank_triples` (``sides``, ``ties``, ``batch``, ``cands``)."""
    src, rel, dst = test
    ranks = rank_triples(model, src, rel, dst, known=known, **kw)
    ks = tuple(int(k) for k in ks)
    sums = {s: rank_sums(r, ks) for s, r in ranks.items()}
    res = metrics_from_sums(sum(sums.values()), ks)
    for s, v in sums.items():
        res[s] = metrics_from_sums(v, ks)
    res["n"] = int(torch.as_tensor(src).numel())
    return res
