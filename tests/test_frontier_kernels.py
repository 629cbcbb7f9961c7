"""Row sets of frontier inference (csrc/hip/frontier.hip, ops/frontier_ops.py) against numpy, the
full-neighbourhood layer over a set's compact table (csrc/hip/sage_csr.hip through
csr_rowset.h's RowRank) against the same layer on the full table, bit for bit, and the binding
discipline of the submodule ``_hip_ops.frontier`` (docs/DESIGN.md 9j).  Every GPU test has an
unmarked CPU twin on the torch implementations.
"""
import itertools

import numpy as np
import pytest
import torch

from test_binding_validation import _named, _ring, _strided, _wrong_dtype, bf, f32, i32, i64
from test_sage_csr_kernels import graph_of, make_csr

# ----------------------------------------------------------------------------------------- 1. sets


def np_closure(csr, T, N, rows, mask):
    """np.unique of the valid rows and their valid masked neighbours"""
    indptr, nbr, _ = csr
    r = np.unique(np.asarray(rows, np.int64))
    r = r[(r >= 0) & (r < N)]
    parts = [r]
    for v in r:
        for t in range(T):
            if (mask >> t) & 1:
                parts.append(nbr[indptr[v * T + t]:indptr[v * T + t + 1]].astype(np.int64))
    j = np.concatenate(parts)
    return np.unique(j[(j >= 0) & (j < N)])


def set_case(N, seed=0):
    """two edge types, degrees 0..5, neighbour entries of -1 and N written into the CSR; the
    row list has duplicates, -1 and N"""
    rng = np.random.default_rng(seed + N)
    d = rng.integers(0, 6, (N, 2))
    d[0] = (2, 2)
    indptr, nbr, w = make_csr(rng, N, 2, lambda r, t: int(d[r, t]), lambda n: rng.uniform(0.5, 1.5, n))
    nbr = nbr.copy()
    nbr[0], nbr[-1] = -1, N
    if nbr.size > 4:
        nbr[nbr.size // 2] = N
    k = max(1, N // 4)
    rows = np.concatenate([rng.integers(0, N, k), [-1, N, 0, 0], rng.integers(0, N, 2)])
    return (indptr, nbr, w), rows


def check_set(s, want, N):
    """the list is sorted and equal to the numpy set, rank[w] is the number of set bits before
    word w, positions(list) == arange(count)"""
    W = (N + 31) // 32
    assert s.count == len(want) and s.num_rows == N
    assert s.rows.dtype == torch.int32 and tuple(s.table.shape) == (W, 2) and s.table.dtype == torch.int32
    got = s.rows.cpu().numpy()
    assert np.array_equal(got, want)  # np.unique is sorted
    bits = np.zeros(W, np.uint32)
    np.bitwise_or.at(bits, want >> 5, (np.uint32(1) << (want & 31).astype(np.uint32)))
    assert np.array_equal(s.words.contiguous().cpu().numpy().view(np.uint32), bits)
    pop = np.array([bin(int(b)).count("1") for b in bits], np.int64)
    assert np.array_equal(s.rank.cpu().numpy().astype(np.int64), np.cumsum(pop) - pop)
    assert torch.equal(s.positions(s.rows).cpu(), torch.arange(s.count))
    absent = np.setdiff1d(np.arange(-1, N + 1), want)
    assert bool((s.positions(torch.from_numpy(absent)) == -1).all())


def _sets_against_numpy(device, N, mask):
    from euler_amd.ops.frontier_ops import neighbor_closure, row_set

    csr, rows = set_case(N)
    g = graph_of(csr, 2, device)
    check_set(neighbor_closure(g, torch.from_numpy(rows).to(device), mask), np_closure(csr, 2, N, rows, mask), N)
    check_set(row_set(g, torch.from_numpy(rows).to(device)), np_closure(csr, 2, N, rows, 0), N)


_SET_N = [1, 31, 32, 33, 200]


@pytest.mark.parametrize("mask", [1, 2, 3])
@pytest.mark.parametrize("N", _SET_N)
def test_sets_against_numpy_cpu(N, mask):
    _sets_against_numpy("cpu", N, mask)


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [1, 2, 3])
@pytest.mark.parametrize("N", _SET_N)
def test_sets_against_numpy_gpu(cuda, N, mask):
    _sets_against_numpy(cuda, N, mask)


def _empty_row_list(device):
    from euler_amd.ops.frontier_ops import neighbor_closure

    csr, _ = set_case(33)
    s = neighbor_closure(graph_of(csr, 2, device), torch.zeros(0, dtype=torch.int64, device=device), 3)
    check_set(s, np.zeros(0, np.int64), 33)
    assert s.count == 0 and not s.table.any()


def test_empty_row_list_cpu():
    _empty_row_list("cpu")


@pytest.mark.gpu
def test_empty_row_list_gpu(cuda, monkeypatch):
    """count 0 and nothing launched: the ops of the submodule are not even looked up"""
    from euler_amd.ops import frontier_ops

    monkeypatch.setattr(frontier_ops, "_frontier", lambda: pytest.fail("an empty row list launched a kernel"))
    _empty_row_list(cuda)


HUB_N, HUB_A, HUB_B = 6000, 3, 4000  # rows with 300 and 5,000 edges: over the 256-edge hub threshold


def hub_case():
    rng = np.random.default_rng(7)
    deg = {HUB_A: (300, 0), HUB_B: (2000, 3000)}
    csr = make_csr(rng, HUB_N, 2, lambda r, t: deg.get(r, (1, 1))[t], lambda n: np.ones(n))
    rows = np.concatenate([[HUB_A, HUB_B, HUB_A], rng.integers(0, HUB_N, 70)])  # three blocks' worth of listed rows
    return csr, rows


def _hub_rows(device):
    from euler_amd.ops.frontier_ops import neighbor_closure

    csr, rows = hub_case()
    g = graph_of(csr, 2, device)
    for mask in (1, 2, 3):
        want = np_closure(csr, 2, HUB_N, rows, mask)
        check_set(neighbor_closure(g, torch.from_numpy(rows).to(device), mask), want, HUB_N)
    assert len(np_closure(csr, 2, HUB_N, [HUB_B], 3)) > 3000  # the hub's neighbours are the set


def test_hub_rows_cpu():
    _hub_rows("cpu")


@pytest.mark.gpu
def test_hub_rows_gpu(cuda):
    from euler_amd.ops._native import hip

    assert 256 == hip().sage_csr_hub_degree < 300
    _hub_rows(cuda)


# ----------------------------------------------------------------------------------------- 2. mapped layer

LN, LD = 333, 32
L_HUB, L_ZERO_DEG, L_ZERO_W = 7, 11, 19
_MS = [1, 7, 64, 65, 130]


def layer_case():
    """N = 333, T = 2: row L_HUB with 400 + 300 edges, L_ZERO_DEG without any, L_ZERO_W with
    edges of zero weight; 130 targets that start with the hub, the two zero rows, both
    out-of-range values and a duplicate pair (M = 7 has them all)"""
    rng = np.random.default_rng(21)
    d = rng.integers(0, 9, (LN, 2))
    d[L_HUB], d[L_ZERO_DEG], d[L_ZERO_W], d[5] = (400, 300), 0, (3, 2), (3, 3)
    indptr, nbr, w = make_csr(rng, LN, 2, lambda r, t: int(d[r, t]), lambda n: rng.uniform(0.5, 1.5, n))
    w = w.copy()
    w[indptr[L_ZERO_W * 2]:indptr[L_ZERO_W * 2 + 2]] = 0.0
    targets = np.concatenate([[L_HUB, L_ZERO_DEG, L_ZERO_W, -1, LN, 5, 5], rng.integers(0, LN, 123)])
    targets[100] = L_HUB
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(LN, LD, generator=gen)
    W = {H: torch.randn(H, 2 * LD, generator=gen) / (2 * LD) ** 0.5 for H in (64, 128)}
    return (indptr, nbr, w), targets, x, W


_LAYER = {}


def _layer_ctx(device):
    """graph, targets, inputs and the closures per (mask, M), shared by the cases of a device"""
    key = str(device)
    if key not in _LAYER:
        from euler_amd.ops.frontier_ops import neighbor_closure

        csr, targets, x, W = layer_case()
        g = graph_of(csr, 2, device)
        t = torch.from_numpy(targets).to(device)
        sets = {(mask, M): neighbor_closure(g, t[:M], mask) for mask in (1, 2, 3) for M in _MS}
        for (mask, M), s in sets.items():
            assert np.array_equal(s.rows.cpu().numpy(), np_closure(csr, 2, LN, targets[:M], mask))
        _LAYER[key] = (g, t, x.to(device), {H: w.to(device) for H, w in W.items()}, sets)
    return _LAYER[key]


@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("x_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Hp", [64, 128])
def test_mapped_layer_equals_unmapped_bitwise_gpu(cuda, Hp, x_dtype, out_dtype):
    """S = rows ∪ N(rows), x_c = x[S.rows]: the layer over (x_c, S) and over the full x give
    the same bits — over relu, self_scale, the masks and M, with a hub, a zero-degree and a
    zero-weight target, out-of-range targets and duplicates"""
    from euler_amd.ops.sage_csr_ops import sage_csr_layer

    g, t, x, W, sets = _layer_ctx(cuda)
    xd, Wd = x.to(x_dtype), W[Hp].to(torch.bfloat16)
    for relu, ss, mask, M in itertools.product((True, False), (0.0, 0.25), (1, 2, 3), _MS):
        s = sets[(mask, M)]
        kw = dict(mask=mask, rows=t[:M], nbr_scale=0.75, self_scale=ss, relu=relu, out_dtype=out_dtype)
        full = sage_csr_layer(g, xd, Wd, **kw)
        got = sage_csr_layer(g, xd[s.rows.long()].contiguous(), Wd, x_set=s, **kw)
        assert got.dtype == out_dtype and tuple(got.shape) == (M, Hp)
        assert torch.equal(got, full), (relu, ss, mask, M)
        if M >= 7:
            assert not got[3].any() and not got[4].any() and got[0].any()  # the out-of-range targets, the hub
    # a superset serves too (mask 3's closure under a mask-1 layer), and a caller's out buffer
    s = sets[(3, 130)]
    kw = dict(mask=1, rows=t, nbr_scale=0.75, self_scale=0.25, out_dtype=out_dtype)
    out = torch.empty(130, Hp, dtype=out_dtype, device=cuda)
    sage_csr_layer(g, xd[s.rows.long()].contiguous(), Wd, x_set=s, out=out, **kw)
    assert torch.equal(out, sage_csr_layer(g, xd, Wd, **kw))


@pytest.mark.parametrize("Hp", [64, 128])
def test_mapped_layer_equals_unmapped_cpu(Hp):
    """the CPU twin: the composed layer with col / src remapped through positions against the
    composed layer on the full table (fp32: the sums run in the same order, 1e-6 covers the rest)"""
    from euler_amd.ops.sage_csr_ops import sage_csr_layer

    g, t, x, W, sets = _layer_ctx("cpu")
    for relu, ss, mask, M in itertools.product((True, False), (0.0, 0.25), (1, 2, 3), _MS):
        s = sets[(mask, M)]
        kw = dict(mask=mask, rows=t[:M], nbr_scale=0.75, self_scale=ss, relu=relu, out_dtype=torch.float32,
                  impl="composed")
        full = sage_csr_layer(g, x, W[Hp], **kw)
        got = sage_csr_layer(g, x[s.rows.long()], W[Hp], x_set=s, **kw)
        assert tuple(got.shape) == (M, Hp)
        assert torch.allclose(got, full, rtol=1e-6, atol=1e-6), (relu, ss, mask, M)
    with pytest.raises(ValueError, match="x_set.count"):
        sage_csr_layer(g, x, W[Hp], x_set=sets[(1, 7)], impl="composed")


# ----------------------------------------------------------------------------------------- 3. a missing row


def _missing_row_is_refused(device, impl, named):
    """a set that lacks one neighbour of a target: refused by name, nothing read through it,
    and the next well-formed call is right"""
    from euler_amd.ops.frontier_ops import row_set
    from euler_amd.ops.sage_csr_ops import sage_csr_layer

    g, t, x, W, sets = _layer_ctx(device)
    dt = torch.bfloat16 if impl == "fused" else torch.float32
    xd, Wd = x.to(dt), W[64].to(dt)
    full = sets[(3, 7)]
    indptr, nbr = g.indptr.cpu().numpy(), g.nbr.cpu().numpy()
    victim = int(nbr[indptr[5 * 2]])  # a neighbour of target row 5 that carries weight
    assert victim not in (L_HUB, L_ZERO_DEG, L_ZERO_W, 5)
    short = row_set(g, full.rows[full.rows != victim])
    assert short.count == full.count - 1
    kw = dict(mask=3, rows=t[:7], nbr_scale=0.75, self_scale=0.25, out_dtype=dt, impl=impl)
    with pytest.raises(RuntimeError, match=named):
        sage_csr_layer(g, xd[short.rows.long()].contiguous(), Wd, x_set=short, **kw)
    # a set without a target's own row is refused the same way
    no_self = row_set(g, full.rows[full.rows != 5])
    with pytest.raises(RuntimeError, match=named):
        sage_csr_layer(g, xd[no_self.rows.long()].contiguous(), Wd, x_set=no_self, **kw)
    got = sage_csr_layer(g, xd[full.rows.long()].contiguous(), Wd, x_set=full, **kw)
    want = sage_csr_layer(g, xd, Wd, **kw)
    assert torch.equal(got, want) if impl == "fused" else torch.allclose(got, want, rtol=1e-6, atol=1e-6)


def test_missing_row_is_refused_cpu():
    _missing_row_is_refused("cpu", "composed", "sage_csr_layer")


@pytest.mark.gpu
def test_missing_row_is_refused_gpu(cuda):
    _missing_row_is_refused(cuda, "fused", "sage_csr_fwd_mapped")


@pytest.mark.gpu
def test_gpu_composed_with_a_set_is_refused(cuda):
    from euler_amd.ops.sage_csr_ops import sage_csr_layer

    g, t, x, W, sets = _layer_ctx(cuda)
    s = sets[(1, 7)]
    with pytest.raises(ValueError, match="CPU path"):
        sage_csr_layer(g, x[s.rows.long()].to(torch.bfloat16), W[64].to(torch.bfloat16), mask=1, rows=t[:7], x_set=s,
                       impl="composed")


# ----------------------------------------------------------------------------------------- 4. bindings
# one row per callable of _hip_ops.frontier: (builder of well-typed CPU arguments, the operand the
# op checks first: its anchor)


def _f():
    from euler_amd.ops._native import hip

    return hip().frontier


F_ROWS = {
    "mark_rows": (lambda: (i32(1, 2), i32(4), 8), "set_words"),
    "mark_neighbors": (lambda: (i32(1, 2), i64(9), i32(4), 1, 1, i32(4)), "set_words"),
    "rank_words": (lambda: (i32(1, 2), 8), "set_words"),
    "list_rows": (lambda: (i32(1, 2), 8, 0), "set_words"),
    "sage_csr_fwd_mapped": (lambda: (i64(9), i32(4), f32(4), 1, 1, bf(2, 16), i32(1, 2), 2, i32(1), bf(64, 32)), "x"),
}


def test_frontier_table_covers_every_export():
    f = _f()
    assert set(F_ROWS) == {n for n in dir(f) if not n.startswith("_")}
    assert all(callable(getattr(f, n)) for n in F_ROWS)
    from euler_amd.ops._native import hip

    assert not callable(hip().frontier) and not any(hasattr(hip(), n) for n in F_ROWS)  # only on the submodule


@pytest.mark.parametrize("name", sorted(F_ROWS))
def test_frontier_cpu_operands_are_refused_by_name(name):
    build, first = F_ROWS[name]
    with pytest.raises(RuntimeError) as e:
        getattr(_f(), name)(*build())
    assert _named(str(e.value), name, first), str(e.value)


def _f_samples(dev):
    """one well-formed call per op on a ring of 8 rows: (op, operands by the binding's names,
    call).  The set ops write set_words in place and are idempotent (or-ing bits, recomputing
    ranks), so a repeated call leaves the same bits."""
    indptr, nbr, cumw = _ring(dev)
    rows = torch.tensor([1, 6, 6], dtype=torch.int32, device=dev)
    marked = torch.tensor([[0b11001111, 0]], dtype=torch.int32, device=dev)  # rows 1, 6, their neighbours 2, 3, 7, 0
    ranked = marked.clone()  # one word: its rank is 0
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 16, generator=g).to(dev).to(torch.bfloat16)
    W = torch.randn(64, 32, generator=g).to(dev).to(torch.bfloat16)
    return [
        ("mark_rows", {"set_words": torch.zeros(1, 2, dtype=torch.int32, device=dev), "rows": rows},
         lambda f, o: [f.mark_rows(o["set_words"], o["rows"], 8), o["set_words"].clone()][1:]),
        ("mark_neighbors",
         {"set_words": torch.zeros(1, 2, dtype=torch.int32, device=dev), "indptr": indptr, "nbr": nbr, "rows": rows},
         lambda f, o: [f.mark_neighbors(o["set_words"], o["indptr"], o["nbr"], 1, 1, o["rows"]),
                       o["set_words"].clone()][1:]),
        ("rank_words", {"set_words": marked},
         lambda f, o: [f.rank_words(o["set_words"], 8), o["set_words"].clone()]),
        ("list_rows", {"set_words": ranked}, lambda f, o: [f.list_rows(o["set_words"], 8, 6)]),
        ("sage_csr_fwd_mapped",
         {"indptr": indptr, "nbr": nbr, "cumw": cumw, "x": x, "set_words": ranked,
          "missing": torch.zeros(1, dtype=torch.int32, device=dev), "W": W, "rows": rows[:1]},
         lambda f, o: [f.sage_csr_fwd_mapped(o["indptr"], o["nbr"], o["cumw"], 1, 1, o["x"], o["set_words"], 6,
                                             o["missing"], o["W"], o["rows"]), o["missing"].clone()]),
    ]


def test_frontier_samples_cover_every_op():
    assert [s[0] for s in _f_samples("cpu")] == list(F_ROWS)


def _refused(call, f, ops, name, bad, op):
    with pytest.raises(RuntimeError) as e:
        call(f, {**ops, name: bad})
    assert _named(str(e.value), op, name), str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(5))
def test_frontier_each_operand_spoiled_is_refused_and_the_op_still_gives_the_same_bits(cuda, k):
    f = _f()
    op, ops, call = _f_samples(cuda)[k]
    before = [t.clone() for t in call(f, ops)]
    if op == "mark_rows":
        assert before[0].tolist() == [[0b01000010, 0]]
    if op == "mark_neighbors":
        assert before[0].tolist() == [[0b10001101, 0]]
    if op == "list_rows":
        assert before[0].tolist() == [0, 1, 2, 3, 6, 7]
    if op == "rank_words":
        assert before[0].tolist() == [6]
    if op == "sage_csr_fwd_mapped":
        assert before[1].tolist() == [0] and before[0].any()
    for name, t in ops.items():
        _refused(call, f, ops, name, _wrong_dtype(t), op)
        _refused(call, f, ops, name, t.cpu(), op)
        if t.numel() > 1:  # a one-element tensor has no strided form
            _refused(call, f, ops, name, _strided(t), op)
        if torch.cuda.device_count() >= 2:  # with the anchor moved, the next operand is the one named
            with pytest.raises(RuntimeError) as e:
                call(f, {**ops, name: t.to("cuda:1")})
            assert op in str(e.value) and "cuda:" in str(e.value), str(e.value)
    after = call(f, ops)
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))


@pytest.mark.gpu
def test_mapped_binding_checks_the_table_height(cuda):
    f = _f()
    _, ops, call = _f_samples(cuda)[4]
    with pytest.raises(RuntimeError, match="sage_csr_fwd_mapped: x must have count"):
        call(f, {**ops, "x": ops["x"][:5].contiguous()})
