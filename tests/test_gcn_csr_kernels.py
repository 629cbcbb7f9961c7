"""The fused full-neighbourhood GCN-family layer (csrc/hip/gcn_csr.hip, ops/gcn_csr_ops.py)
against an fp64 dense-adjacency reference.

Rounding points of the kernel (bf = round to bf16, RNE): A = bf(a * (sum_e b x (+ b x_self))) with
the sum in fp32, W is bf16, out = cast(c * act(A @ W^T)).  For real-valued data the conditions
(a)-(c) of tests/test_sage_csr_kernels.py (check_abc) hold against ``o``, the reference rounded
at those points, and ``f``, the unrounded one.
"""
import numpy as np
import pytest
import torch

from test_sage_csr_kernels import bf, check_abc, graph_of, make_csr

# (c)'s absolute term = 4 x the largest excess max(|k - o| - 2^-7 |o|) of the kernel against the
# oracle, measured over seeds 0..4 and the three masks on an MI355X (every figure:
# profiles/gcn_infer/oracle_margins.json); the same bound covers fused against composed.
# The excess comes from outputs next to the ReLU zero, where one bf16 flip of an A element moves
# a pre-activation across it.  Measured: kernel vs oracle 2.316e-3 (RMS ratios 0.057 - 0.195,
# shares 0.14 % - 1.35 %); for information, fused vs composed 2.869e-3 (RMS ratios 0.058 - 0.240,
# shares to 1.48 %).
MEASURED_KERNEL_EXCESS = 0.002315521240234375
ATOL = 4.0 * MEASURED_KERNEL_EXCESS

N, HUB, EMPTY, P, Q = 200, 7, 11, 20, 21


def adjacency(csr, T, mask):
    """[N, N] fp64 edge counts of the masked types (neighbours outside [0, N) dropped)"""
    indptr, nbr, _ = csr
    n = (len(indptr) - 1) // T
    A = np.zeros((n, n))
    for r in range(n):
        for t in range(T):
            js = nbr[indptr[r * T + t]:indptr[r * T + t + 1]] if (mask >> t) & 1 else nbr[:0]
            np.add.at(A[r], js[(js >= 0) & (js < n)], 1)
    return torch.from_numpy(A)


def dense_layer(A, x, W, a, b, c, self_loop, relu, rounded, out_bf16=True):
    """c * act((a * ((A + I) (b * x))) @ W^T) in fp64; ``rounded``: bf16 at A and at the output"""
    xb = x.double() if b is None else x.double() * b.double().view(-1, 1)
    t = a.double().view(-1, 1) * ((A + torch.eye(A.shape[0], dtype=torch.float64) * int(self_loop)) @ xb)
    if rounded:
        t = bf(t.float()).double()
    y = t @ W.double().t()
    y = torch.relu(y) if relu else y
    y = y if c is None else y * c.double().view(-1, 1)
    return bf(y.float()).double() if rounded and out_bf16 else y


def small_graph(seed, weight):
    """200 rows, 2 edge types, <= 2 edges per segment; row HUB lists P and Q 150 times each and
    P three times more (303 edges of type 0), row EMPTY lists nothing, one neighbour is N"""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 3, (N, 2))
    d[HUB], d[EMPTY] = (303, 1), 0
    indptr, nbr, w = make_csr(rng, N, 2, lambda r, t: int(d[r, t]), weight)
    h = int(indptr[HUB * 2])
    nbr[h:h + 303] = np.array([P, Q] * 150 + [P] * 3, np.int32)
    nbr[int(indptr[3 * 2 + 2]) - 1 if d[3].sum() else h + 303] = N
    return indptr, nbr, w


_EXACT = {}


def exact_case(Dp, Hp):
    """small integers and power-of-two scales: every value at every rounding point is exact in
    bf16, every fp32 sum exact in any order (the hub's 300 terms cancel pairwise: x[Q] = -x[P])"""
    if (Dp, Hp) not in _EXACT:
        rng = np.random.default_rng(3)
        csr = small_graph(3, lambda n: np.ones(n))
        x = torch.from_numpy(rng.integers(-1, 2, (N, Dp))).float()
        x[Q] = -x[P]
        W = torch.zeros(Hp, Dp)
        for h in range(Hp):
            W[h, rng.choice(Dp, 2, replace=False)] = torch.from_numpy(rng.integers(-1, 2, 2)).float()
        a, b, c = (torch.from_numpy(2.0 ** rng.integers(lo, hi, N)).float() for lo, hi in ((-1, 1), (-1, 2), (-1, 2)))
        b[Q] = b[P]
        rows = rng.integers(0, N, 70)
        rows[:4], rows[69] = (HUB, EMPTY, 3, 5), 5
        _EXACT[(Dp, Hp)] = (csr, x, W, a, b, c, torch.from_numpy(rows))
    return _EXACT[(Dp, Hp)]


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("self_loop", [True, False])
@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Hp", [64, 128])
@pytest.mark.parametrize("Dp", [16, 48, 128, 512])  # 48: Dp / 8 no power of two; 512: LDS past 64 KiB
def test_exact_data_bitwise(cuda, Dp, Hp, dtype, with_b, with_c, self_loop, relu):
    from euler_amd.ops._native import hip
    from euler_amd.ops.gcn_csr_ops import gcn_csr_layer

    csr, x, W, a, b, c, rows = exact_case(Dp, Hp)
    mask = 3 if relu else 1  # type 1 masked out in half of the cases
    # one full tile plus a tail of 6: the 70 listed rows (hub, empty, duplicate, the row with the
    # out-of-range neighbour), then as many more as the kernel's tile takes beyond 64
    tile = hip().gcn_csr.tile_rows
    rows = torch.cat([rows, (torch.arange(tile + 6 - len(rows)) * 7 + 1) % N])
    assert 303 > hip().sage_csr_hub_degree and len(rows) == tile + 6 >= 70
    b, c = (b if with_b else None), (c if with_c else None)
    A = adjacency(csr, 2, mask)
    want = dense_layer(A, x, W, a, b, c, self_loop, relu, False)
    # what makes "bitwise" legitimate: rounding at the kernel's rounding points changes nothing
    assert torch.equal(dense_layer(A, x, W, a, b, c, self_loop, relu, True), want)
    dev = lambda t: None if t is None else t.to(cuda)  # noqa: E731
    out = gcn_csr_layer(graph_of(csr, 2, cuda), x.to(cuda, dtype), W.to(cuda, torch.bfloat16), mask=mask,
                        rows=rows.to(cuda), tgt_scale=dev(a), src_scale=dev(b), out_scale=dev(c),
                        self_loop=self_loop, relu=relu, out_dtype=dtype)
    assert out.dtype == dtype and tuple(out.shape) == (tile + 6, Hp)
    assert torch.equal(out.double().cpu(), want[rows])


_REAL = {}


def real_case(seed=0, D=128, H=128):
    if seed not in _REAL:
        rng = np.random.default_rng(seed)
        csr = small_graph(seed, lambda n: rng.uniform(0.5, 1.5, n))
        gen = torch.Generator().manual_seed(seed)
        x = torch.randn(N, D, generator=gen).to(torch.bfloat16)
        W = (torch.randn(H, D, generator=gen) / D ** 0.5).to(torch.bfloat16)
        _REAL[seed] = (csr, x, W, {})
    return _REAL[seed]


def real_oracles(seed, mask):
    """(o, f, a, b): the reference with the true GCN scales (a from the offsets, b from the
    adjacency's column sums, self loops counted), rounded as the kernel and unrounded"""
    csr, x, W, ref = real_case(seed)
    if mask not in ref:
        A = adjacency(csr, 2, mask)
        deg_t = (np.diff(csr[0]).reshape(N, 2) * [(mask >> t) & 1 for t in range(2)]).sum(1)
        a, b = torch.from_numpy((deg_t + 1.0) ** -0.5).float(), (A.sum(0) + 1.0).rsqrt().float()
        ref[mask] = tuple(dense_layer(A, x, W, a, b, b, True, True, r).float() for r in (True, False)) + (a, b)
    return ref[mask]


def real_run(g, x, W, mask, impl="fused", rows=None, out_dtype=torch.bfloat16):
    from euler_amd.ops.gcn_csr_ops import gcn_csr_layer, gcn_scales

    a, b = gcn_scales(g, mask, True)
    return gcn_csr_layer(g, x.to(g.device), W.to(g.device), mask=mask, rows=rows, tgt_scale=a, src_scale=b,
                         out_scale=b, impl=impl, out_dtype=out_dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [1, 2, 3])
def test_real_data_against_oracle(cuda, mask):
    csr, x, W, _ = real_case()
    from euler_amd.ops.gcn_csr_ops import gcn_scales

    o, f, a, b = real_oracles(0, mask)
    g = graph_of(csr, 2, cuda)
    for got, want in zip(gcn_scales(g, mask, True), (a, b)):  # rsqrt on the device: one fp32 ulp
        assert torch.allclose(got.cpu(), want, rtol=2.0 ** -22, atol=0)
    k = real_run(g, x, W, mask)
    check_abc(k, o, f, ATOL, f"gcn real mask {mask}")
    check_abc(k, real_run(g, x, W, mask, "composed").float().cpu(), f, ATOL, f"gcn a/b mask {mask}")


@pytest.mark.gpu
def test_two_launches_bit_identical(cuda):
    csr, x, W, _ = real_case()
    g = graph_of(csr, 2, cuda)
    for mask in (1, 3):
        assert torch.equal(real_run(g, x, W, mask), real_run(g, x, W, mask))


@pytest.mark.gpu
def test_guards(cuda):
    """bad widths, dtype mismatches and a rows entry outside [0, N) are refused by the binding
    (a RuntimeError naming gcn_csr_fwd), before any launch"""
    from euler_amd.ops.gcn_csr_ops import gcn_csr_layer

    csr, x, W, a, b, c, rows = exact_case(16, 64)
    g = graph_of(csr, 2, cuda)
    xd, Wd, ad = x.to(cuda, torch.bfloat16), W.to(cuda, torch.bfloat16), a.to(cuda)
    ok = dict(tgt_scale=ad, rows=rows.to(cuda))
    gcn_csr_layer(g, xd, Wd, **ok)
    bad = [dict(ok, x=torch.zeros(N, 24, device=cuda, dtype=torch.bfloat16), w=Wd.new_zeros(64, 24)),  # Dp % 16
           dict(ok, w=Wd[:32].contiguous()),  # Hp % 64
           dict(ok, w=Wd.float()), dict(ok, tgt_scale=ad.double()), dict(ok, src_scale=ad.half()),  # dtypes
           dict(ok, tgt_scale=ad[:-1].contiguous()), dict(ok, out=torch.zeros(70, 64, device=cuda)),
           dict(ok, rows=torch.tensor([3, N], device=cuda)), dict(ok, rows=torch.tensor([-1, 3], device=cuda))]
    for kw in bad:
        with pytest.raises(RuntimeError, match="gcn_csr_fwd"):
            gcn_csr_layer(g, kw.pop("x", xd), kw.pop("w", Wd), **kw)
    with pytest.raises(ValueError, match="weight must be"):
        gcn_csr_layer(g, xd, Wd.new_zeros(64, 32), **ok)


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [1, 2, 3])
def test_degrees_match_bincount(cuda, mask):
    from euler_amd.ops.gcn_csr_ops import gcn_degrees

    indptr, nbr, _ = csr = small_graph(0, lambda n: np.ones(n))
    seg = np.diff(indptr)
    on = np.tile([(mask >> t) & 1 == 1 for t in range(2)], N)
    j = torch.from_numpy(nbr[np.repeat(on, seg)]).long()
    deg_t, deg_s = gcn_degrees(graph_of(csr, 2, cuda), mask)
    assert deg_t.dtype == deg_s.dtype == torch.int32
    assert torch.equal(deg_t.cpu().long(), torch.from_numpy((seg * on).reshape(N, 2).sum(1)))
    assert torch.equal(deg_s.cpu().long(), torch.bincount(j[(j >= 0) & (j < N)], minlength=N))


def test_composed_cpu_matches_dense_oracle():
    """the composed implementation on a CPU graph (its fp32 form: fp32 weights) against the
    unrounded fp64 reference, for every row and for a row list"""
    csr, x, W, _ = real_case()
    g = graph_of(csr, 2, "cpu")
    rows = torch.tensor([HUB, EMPTY, 5, 5, 199, 0])
    for mask in (1, 2, 3):
        f = real_oracles(0, mask)[1]
        y = real_run(g, x.float(), W.float(), mask, "composed", out_dtype=torch.float32)
        assert torch.allclose(y, f, rtol=1e-5, atol=1e-5)
        yr = real_run(g, x.float(), W.float(), mask, "composed", rows, torch.float32)
        assert torch.allclose(yr, f[rows], rtol=1e-5, atol=1e-5)
    with pytest.raises(RuntimeError, match="gfx950 kernel"):
        real_run(g, x, W, 1)
