"""DeviceGraph.from_edges: edge list -> per-(row, type) CSR (ops/graph_build_ops.py,
csrc/hip/graph_build.hip).

Oracle: ``numpy.lexsort`` by (row * T + type, dst, input index), then ``DeviceGraph.from_csr``
on the sorted arrays.  ``indptr`` and ``nbr`` must be equal; ``cumw`` must be within 1 fp32
ulp of the float64 sequential per-segment prefix sum cast to float32 (fp64 accumulation
leaves an error far below half an fp32 ulp, so only a double-rounding tie can move the
result, and then by one ulp).  The CPU runs check the torch twin, the GPU runs the kernels
(against the same oracle, and against the twin for ``indptr`` / ``nbr`` / edge order).
"""
import functools

import numpy as np
import pytest
import torch

from euler_amd.graph.device_graph import DeviceGraph

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


# ----------------------------------------------------------------------------- oracle
def _oracle(src, dst, w, et, N, T, symmetric=False, duplicates="keep"):
    """(indptr, nbr, weights, ref_cumw fp32, order) by lexsort; rows are the ids"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    E = len(src)
    w = np.ones(E, np.float32) if w is None else np.asarray(w, np.float32)
    et = np.zeros(E, np.int64) if et is None else np.asarray(et, np.int64)
    if symmetric:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
        w, et = np.concatenate([w, w]), np.concatenate([et, et])
    seg = src * T + et
    order = np.lexsort((np.arange(len(seg)), dst, seg))
    seg, nbr, w = seg[order], dst[order], w[order]
    if duplicates == "sum" and len(seg):
        head = np.ones(len(seg), bool)
        head[1:] = (seg[1:] != seg[:-1]) | (nbr[1:] != nbr[:-1])
        starts = np.flatnonzero(head)
        ends = np.append(starts[1:], len(seg))
        # fp64 sum in input order (np.cumsum-free: a plain sequential loop per run)
        merged = np.empty(len(starts), np.float32)
        for k, (a, b) in enumerate(zip(starts, ends)):
            acc = 0.0
            for x in w[a:b]:
                acc += float(x)
            merged[k] = np.float32(acc)
        seg, nbr, w, order = seg[starts], nbr[starts], merged, order[starts]
    indptr = np.searchsorted(seg, np.arange(N * T + 1)).astype(np.int64)
    ref = np.empty(len(w), np.float32)
    for s in np.flatnonzero(np.diff(indptr)):
        a, b = indptr[s], indptr[s + 1]
        ref[a:b] = np.cumsum(w[a:b].astype(np.float64)).astype(np.float32)  # sequential fp64
    return indptr, nbr.astype(np.int32), w, ref, order


def _ulps(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max()) if len(a) else 0


def _check(g, orc, T, exact=False):
    indptr, nbr, w, ref, _ = orc
    gc = DeviceGraph.from_csr(indptr, nbr, w, T, device="cpu")
    assert g.num_types == T and g.indptr.dtype == torch.int64 and g.nbr.dtype == torch.int32
    assert g.cumw.dtype == torch.float32
    assert torch.equal(g.indptr.cpu(), gc.indptr)
    assert torch.equal(g.nbr.cpu(), gc.nbr)
    u = _ulps(g.cumw.cpu().numpy(), ref)
    print("cumw max ulp distance to the fp64 sequential reference:", u)
    assert u <= 1
    if exact:
        assert torch.equal(g.cumw.cpu(), gc.cumw)
        assert u == 0
    return gc


# ----------------------------------------------------------------------------- cases
def _dyadic(rng, n):
    return (rng.integers(0, 256, n) * 0.25).astype(np.float32)  # multiples of 0.25 below 64


@functools.lru_cache(maxsize=None)
def _base(dyadic=False):
    """N = 300, T = 2, E ~ 2,400, dst from 40 values on some rows (duplicates), row 7 has no
    edges, random order"""
    rng = np.random.default_rng(5)
    N, T, E = 300, 2, 2400
    src = rng.integers(0, N, E)
    src[src == 7] = 8
    dst = rng.integers(0, N, E)
    few = src % 3 == 0
    dst[few] = rng.integers(0, 40, int(few.sum()))
    et = rng.integers(0, T, E)
    w = _dyadic(rng, E) if dyadic else (0.1 + rng.random(E)).astype(np.float32)
    p = rng.permutation(E)
    return src[p], dst[p], w[p], et[p], N, T


@functools.lru_cache(maxsize=None)
def _random(E, N, T, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, N, E), rng.integers(0, N, E), (0.1 + rng.random(E)).astype(np.float32),
            rng.integers(0, T, E), N, T)


@functools.lru_cache(maxsize=None)
def _regimes(dyadic=False):
    """segments of exactly 64, 65, 256, 257 and 5,000 edges (rows 0 .. 4) among short ones:
    the lane / wave / block regimes of the prefix kernel and their boundaries"""
    rng = np.random.default_rng(11)
    N = 700
    lens = [64, 65, 256, 257, 5000]
    src = np.concatenate([np.full(n, r) for r, n in enumerate(lens)] + [rng.integers(5, N, 1500)])
    E = len(src)
    dst = rng.integers(0, N, E)
    w = _dyadic(rng, E) if dyadic else (0.1 + rng.random(E)).astype(np.float32)
    p = rng.permutation(E)
    case = (src[p], dst[p], w[p], None, N, 1)
    deg = np.bincount(case[0], minlength=N)
    assert list(deg[:5]) == lens
    return case


def _build(case, device, **kw):
    src, dst, w, et, N, T = case
    return DeviceGraph.from_edges(src, dst, w, et, num_types=T, num_nodes=N, device=device, **kw)


# ----------------------------------------------------------------------------- structure
@pytest.mark.parametrize("device", DEVICES)
def test_base_graph_matches_oracle(device):
    case = _base()
    g = _build(case, device)
    _check(g, _oracle(*case), case[5])
    assert int(g.degree(torch.tensor([7], device=g.device))) == 0


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("E", [0, 1, 257])
def test_tiny_edge_counts(device, E):
    case = _random(E, 50, 2, seed=E)
    _check(_build(case, device), _oracle(*case), 2)


@pytest.mark.parametrize("device", DEVICES)
def test_several_sort_tiles(device):
    case = _random(70001, 5000, 1, seed=3)
    _check(_build(case, device), _oracle(*case), 1)


@pytest.mark.parametrize("device", DEVICES)
def test_single_node(device):
    rng = np.random.default_rng(2)
    case = (np.zeros(9, np.int64), np.zeros(9, np.int64), rng.random(9).astype(np.float32), None, 1, 1)
    g = _build(case, device)
    _check(g, _oracle(*case), 1)
    assert g.num_rows == 1 and g.num_edges == 9


@pytest.mark.parametrize("device", DEVICES)
def test_thirty_two_types(device):
    case = _random(3000, 40, 32, seed=4)
    g = _build(case, device)
    _check(g, _oracle(*case), 32)
    g2 = DeviceGraph.from_edges(case[0], case[1], case[2], case[3], num_nodes=40, device=device)
    assert g2.num_types == 32  # max + 1


@pytest.mark.parametrize("device", DEVICES)
def test_prefix_regimes_and_boundaries(device):
    case = _regimes()
    g = _build(case, device)
    _check(g, _oracle(*case), 1)
    assert g.degree(torch.arange(5, device=g.device)).tolist() == [64, 65, 256, 257, 5000]


@pytest.mark.parametrize("device", DEVICES)
def test_int32_ids_and_device_inputs(device):
    src, dst, w, et, N, T = _base()
    dev = torch.device(device)
    g = DeviceGraph.from_edges(torch.from_numpy(src).int().to(dev), torch.from_numpy(dst).int().to(dev),
                               torch.from_numpy(w).to(dev), torch.from_numpy(et).to(dev), num_types=T, num_nodes=N,
                               device=device)
    _check(g, _oracle(src, dst, w, et, N, T), T)


# ----------------------------------------------------------------------------- exact draws
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("which", ["base", "regimes"])
def test_exact_weights_are_bit_identical_and_draw_alike(device, which):
    """dyadic weights: every prefix sum is exact in fp32, so the arrays equal from_csr's bit
    for bit, and the same seed draws the same neighbours and node2vec walks: the segments are
    sorted the way the bias search needs"""
    case = _base(True) if which == "base" else _regimes(True)
    T = case[5]
    orc = _oracle(*case)
    g = _build(case, device, seed=17)
    _check(g, orc, T, exact=True)
    ref = DeviceGraph.from_csr(orc[0], orc[1], orc[2], T, seed=17, device=device)
    assert torch.equal(g.cumw, ref.cumw) and torch.equal(g.nbr, ref.nbr) and torch.equal(g.indptr, ref.indptr)
    rows = torch.arange(0, g.num_rows, 3, dtype=torch.int32, device=g.device)
    assert torch.equal(g.sample_neighbor(rows, 6), ref.sample_neighbor(rows, 6))
    assert torch.equal(g.random_walk(rows, 5, p=0.5, q=2.0), ref.random_walk(rows, 5, p=0.5, q=2.0))


# ----------------------------------------------------------------------------- options
@pytest.mark.parametrize("device", DEVICES)
def test_duplicates_sum(device):
    case = _base()
    g, order = _build(case, device, duplicates="sum", return_edge_order=True)
    orc = _oracle(*case, duplicates="sum")
    assert len(orc[1]) < len(case[0])  # the case has duplicates to merge
    _check(g, orc, case[5])
    # merged weights: the fp64 sum in input order cast to fp32, bit for bit (the first entry of
    # a segment carries its merged weight itself)
    ip = g.indptr.cpu().numpy()
    first = ip[:-1][ip[:-1] < ip[1:]]
    assert np.array_equal(g.cumw.cpu().numpy()[first], orc[2][first])
    # first-of-run indices
    assert np.array_equal(order.cpu().numpy(), orc[4])


@pytest.mark.parametrize("device", DEVICES)
def test_duplicates_sum_single_entry_segments(device):
    """every segment ends up with one entry, so cumw IS the merged weight: it must equal the
    fp64 sum in input order cast to fp32"""
    rng = np.random.default_rng(9)
    N, E = 37, 4000
    src = rng.integers(0, N, E)
    dst = (src * 7 + 3) % N  # one distinct neighbour per row: runs of ~100 parallel edges
    w = (rng.random(E) * 3).astype(np.float32)
    g = DeviceGraph.from_edges(src, dst, w, num_nodes=N, duplicates="sum", device=device)
    orc = _oracle(src, dst, w, None, N, 1, duplicates="sum")
    assert g.num_edges == len(np.unique(src))
    assert torch.equal(g.nbr.cpu(), torch.from_numpy(orc[1]))
    assert np.array_equal(g.cumw.cpu().numpy(), orc[2])


@pytest.mark.parametrize("device", DEVICES)
def test_keep_preserves_input_order_among_equal_neighbours(device):
    case = _base()
    src, dst, w, et, N, T = case
    g, order = _build(case, device, return_edge_order=True)
    o = order.cpu().numpy()
    assert o.dtype == np.int64 and np.array_equal(np.sort(o), np.arange(len(src)))  # a permutation
    assert np.array_equal(o, _oracle(*case)[4])
    key = (src[o] * T + et[o]) * N + dst[o]
    same = key[1:] == key[:-1]
    assert same.any() and (o[1:][same] > o[:-1][same]).all()
    # src[order] / dst[order] reproduce the CSR
    ip = g.indptr.cpu().numpy()
    seg = np.repeat(np.arange(N * T), np.diff(ip))
    assert np.array_equal(src[o] * T + et[o], seg)
    assert np.array_equal(dst[o], g.nbr.cpu().numpy())


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("duplicates", ["keep", "sum"])
def test_symmetric(device, duplicates):
    case = _base()
    src, dst, w, et, N, T = case
    E = len(src)
    g, order = _build(case, device, symmetric=True, duplicates=duplicates, return_edge_order=True)
    orc = _oracle(*case, symmetric=True, duplicates=duplicates)
    _check(g, orc, T)
    o = order.cpu().numpy()
    assert np.array_equal(o, orc[4])
    assert (o >= E).any() and o.max() < 2 * E
    s2, d2 = np.concatenate([src, dst]), np.concatenate([dst, src])  # reverse copies are E + i
    assert np.array_equal(d2[o], g.nbr.cpu().numpy())
    ip = g.indptr.cpu().numpy()
    assert np.array_equal(s2[o] * T + np.concatenate([et, et])[o], np.repeat(np.arange(N * T), np.diff(ip)))


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, {"duplicates": "sum"}, {"symmetric": True}, {"symmetric": True, "duplicates": "sum"}])
def test_kernels_match_the_cpu_twin(kw):
    for case in (_base(), _regimes()):
        a, oa = _build(case, "cuda", return_edge_order=True, **kw)
        b, ob = _build(case, "cpu", return_edge_order=True, **kw)
        assert torch.equal(a.indptr.cpu(), b.indptr) and torch.equal(a.nbr.cpu(), b.nbr)
        assert torch.equal(oa.cpu(), ob)
        # both are within 1 ulp of the sequential fp64 reference, hence within 2 of each other
        assert _ulps(a.cumw.cpu().numpy(), b.cumw.numpy()) <= 2


# ----------------------------------------------------------------------------- ids
@pytest.mark.parametrize("device", DEVICES)
def test_raw_ids_are_compacted(device):
    rng = np.random.default_rng(21)
    pool = np.unique(rng.integers(0, 1 << 40, 120)).astype(np.int64)
    pool[-1] = (1 << 40) - 1
    used, lonely = pool[:-2], pool[-2:]
    E = 900
    src, dst = rng.choice(used, E), rng.choice(used, E)
    w = (0.1 + rng.random(E)).astype(np.float32)
    seen = np.unique(np.concatenate([src, dst]))
    node_ids = rng.permutation(np.concatenate([seen, lonely]))  # two isolated nodes, any order
    feats = rng.standard_normal((len(node_ids), 6)).astype(np.float32)
    labels = (rng.random((len(node_ids), 3)) > 0.5).astype(np.float32)
    g = DeviceGraph.from_edges(src, dst, w, node_ids=node_ids, features=feats, labels=labels,
                               feature_dtype=torch.float32, device=device)
    ids = np.asarray(g.ids)
    assert ids.dtype == np.uint64 and np.array_equal(ids, np.sort(node_ids).astype(np.uint64))
    assert g.num_rows == len(node_ids)
    rows = g.rows_of(node_ids).numpy()
    assert np.array_equal(ids[rows].astype(np.int64), node_ids)          # round trip
    assert g.rows_of([12345678901234]).tolist() == [-1] or 12345678901234 in node_ids
    assert g.features.dtype == torch.float32 and g.labels.dtype == torch.float32
    assert np.array_equal(g.features.cpu().numpy()[rows], feats)         # tables follow their ids
    assert np.array_equal(g.labels.cpu().numpy()[rows], labels)
    assert g.degree(torch.from_numpy(g.rows_of(lonely).numpy()).to(g.device)).tolist() == [0, 0]
    r_src, r_dst = g.rows_of(src).numpy(), g.rows_of(dst).numpy()
    _check(g, _oracle(r_src, r_dst, w, None, g.num_rows, 1), 1)
    gb = DeviceGraph.from_edges(src, dst, w, node_ids=node_ids, features=feats, device=device)
    assert gb.features.dtype == torch.bfloat16                           # as from_engine stores them


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("bad", [300, -1])
def test_ids_out_of_range_name_the_count(device, bad):
    src, dst, w, et, N, T = _base()
    src = src.copy()
    src[5] = bad
    with pytest.raises(ValueError, match=r"\b1 endpoint ids are outside \[0, 300\)"):
        DeviceGraph.from_edges(src, dst, w, et, num_types=T, num_nodes=N, device=device)
    dst = dst.copy()
    dst[[1, 2]] = bad
    with pytest.raises(ValueError, match=r"\b3 endpoint ids"):
        DeviceGraph.from_edges(src, dst, w, et, num_types=T, num_nodes=N, device=device, duplicates="sum")


# ----------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("device", DEVICES)
def test_refusals(device):
    src, dst, w, et, N, T = _base()
    kw = dict(num_nodes=N, device=device)
    bad = w.copy()
    bad[3] = -0.5
    with pytest.raises(ValueError, match="weights must be finite and >= 0"):
        DeviceGraph.from_edges(src, dst, bad, et, **kw)
    bad[3] = np.nan
    with pytest.raises(ValueError, match="weights must be finite and >= 0"):
        DeviceGraph.from_edges(src, dst, bad, et, **kw)
    bad[3] = np.inf
    with pytest.raises(ValueError, match="weights must be finite and >= 0"):
        DeviceGraph.from_edges(src, dst, bad, et, duplicates="sum", **kw)
    with pytest.raises(ValueError, match=r"edge_type must be in \[0, num_types = 1\)"):
        DeviceGraph.from_edges(src, dst, w, et, num_types=1, **kw)
    with pytest.raises(ValueError, match="num_types = 33.*32"):
        DeviceGraph.from_edges(src, dst, w, et, num_types=33, **kw)
    with pytest.raises(ValueError, match="differ in length"):
        DeviceGraph.from_edges(src, dst[:-1], w, et, **kw)
    with pytest.raises(ValueError, match="differ in length"):
        DeviceGraph.from_edges(src, dst, w[:-1], et, **kw)
    with pytest.raises(ValueError, match="differ in length"):
        DeviceGraph.from_edges(src, dst, w, et[:-1], **kw)
    with pytest.raises(ValueError, match="duplicates must be"):
        DeviceGraph.from_edges(src, dst, w, et, duplicates="max", **kw)
    with pytest.raises(ValueError, match="int32 or int64"):
        DeviceGraph.from_edges(src.astype(np.float32), dst, w, et, **kw)


def test_edge_count_limit_is_checked_before_any_allocation():
    from euler_amd.ops import graph_build_ops as gb

    big = torch.empty(0, dtype=torch.int8).new_empty((1 << 30) + 1, device="meta").long()
    with pytest.raises(ValueError, match=r"2\^31"):
        gb.build_csr(big, big, num_rows=10, symmetric=True)
