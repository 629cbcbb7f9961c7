"""The pipelined stage loop of the routed layer-0 dW (csrc/hip/tree_dw.hip
tr_dw_route_pipe_body; plan key ``dw_route_impl`` = 2, the default).

Every case builds two trainers that differ only in ``EULER_AMD_DW_ROUTE_IMPL`` (2: build, load
and multiply woven into one block per stage; 0: the three phases one after the other) on the
same graph, tables, weights and RNG counter, and asserts that the gradient, the parameters,
the optimizer slots, the loss and the bf16 weight shadows are bitwise equal.  Both bodies give
every accumulator the same MFMAs in the same k order, so nothing may differ.

``EULER_AMD_DW_ROUTE_WG`` forces long slabs on small problems: the plan takes
S = ceil8(ceil(target / tiles)) slabs, at most ceil8(MB), of kps = ceil(MB / S) k-blocks, MB =
layer-0 rows / 32.  A hop has at least 16 slots per parent, so fanouts [7, 3] give MB = B / 2.
A stage is 8 k-blocks.  The shapes are the smallest at which the body takes another path: the
last two stages written out (kps 16), a short last stage (12), less than one stage (3), a short
last slab beside empty ones, exactly one stage on several tiles with 32-slot groups, the loop
of stages that have two more to come (32, the headline's) and the same with a ragged end (28),
two routed problems in one launch, and the pair step.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "benchmarks"))

N = 20_000
PIPE, BASE = 2, 0


def _bits(t):
    return t.detach().reshape(-1).contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), f"{what}: {int((_bits(a) != _bits(b)).sum())} of {a.numel()} words differ"


def _pair(monkeypatch, cuda, B, fanouts, dims, C, route_wg=None, min_kps=None, D=32):
    """two SageTrainers, dw_route_impl = 2 and 0, same graph / tables / weights / RNG counter"""
    from euler_amd.dataset.synthetic import synthetic_features, synthetic_labels
    from euler_amd.graph.device_graph import DeviceGraph
    from euler_amd.models.sage_trainer import SageTrainer

    for key, val in (("EULER_AMD_DW_ROUTE_WG", route_wg), ("EULER_AMD_DW_MIN_KPS", min_kps)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(val))
    feats = synthetic_features(N, D, 2, cuda)
    labels = synthetic_labels(feats, C)
    out = []
    for impl in (PIPE, BASE):
        monkeypatch.setenv("EULER_AMD_DW_ROUTE_IMPL", str(impl))
        g = DeviceGraph.synthetic(N, 8.0, 256, seed=1, device=cuda)
        g.manual_seed(23)
        out.append(SageTrainer(g, B, fanouts, dims, C, features=feats, labels=labels, learning_rate=1e-2,
                               init_seed=5))
    return out


def _check_trainers(a, b):
    a.forward_backward()
    b.forward_backward()
    _same(a.grad, b.grad, "grad")
    assert float(a.grad.abs().sum()) > 0
    for _ in range(3):
        a.step()
        b.step()
    for name in ("flat", "m", "v", "loss_out", "grad"):
        _same(getattr(a, name), getattr(b, name), name)
    shadows = [k for k in a._buf if k.endswith("_sh") or k.endswith("_shT")]
    assert len(shadows) >= 5
    for k in shadows:
        _same(a._buf[k], b._buf[k], k)
    assert torch.isfinite(a.loss_out).all()


def _kps(MB, S):
    return -(-MB // S)


# one 64 x 128 tile (P = 64, Q = 2 D = 64: waves 2 and 3 have no columns and must still build
# their share of G and reach every barrier), fanouts [7, 3]: MB = B / 2
@pytest.mark.gpu
@pytest.mark.parametrize("B,route_wg,S,kps,what", [
    (256, 8, 8, 16, "two full stages: the last two stages written out"),
    (192, 8, 8, 12, "one full stage and a half stage"),
    (96, 16, 16, 3, "less than one stage"),
    (160, 32, 32, 3, "MB = 80: slab 26 holds 2 k-blocks, slabs 27..31 none"),
    (512, 8, 8, 32, "four full stages (the headline's slab): the loop runs twice"),
    (448, 8, 8, 28, "the loop, then a full and a half stage"),
])
def test_one_tile_narrow_q(cuda, monkeypatch, B, route_wg, S, kps, what):
    a, b = _pair(monkeypatch, cuda, B, [7, 3], [64, 64, 32], 5, route_wg=route_wg)
    assert a.plan.splits()[0] == S and b.plan.splits()[0] == S, what
    assert _kps(B // 2, S) == kps, what
    assert a.plan.splits() == b.plan.splits() and a.plan.folds() == b.plan.folds()
    _check_trainers(a, b)


@pytest.mark.gpu
def test_one_stage_two_tiles_32_slot_groups(cuda, monkeypatch):
    """fanouts [25, 10] (32 slots per parent, the headline's groups: a k-block is one group),
    P = 128, Q = 128: MB = 64, 2 tiles, S = 8, kps = 8, exactly one stage"""
    a, b = _pair(monkeypatch, cuda, 64, [25, 10], [128, 128, 64], 16, route_wg=16, D=64)
    assert a.plan.splits()[0] == 8 and b.plan.splits()[0] == 8
    assert _kps(64, 8) == 8
    _check_trainers(a, b)


@pytest.mark.gpu
def test_three_hops_two_routed_problems_in_the_launch(cuda, monkeypatch):
    """both routed problems take the one copy of the body (Q = 32: only wave 0 has columns)"""
    a, b = _pair(monkeypatch, cuda, 64, [3, 2, 2], [64, 64, 64, 32], 8, min_kps=1, D=16)
    assert a.plan.splits() == b.plan.splits() and a.plan.folds() == b.plan.folds()
    assert a.plan.folds()[:2] == [0, 0] and min(a.plan.splits()[:2]) >= 8
    _check_trainers(a, b)


@pytest.mark.gpu
def test_unsupervised_pair_step(cuda, monkeypatch):
    """PairPlan's dW launch: the routed W0 problems of both towers (B = 64 and B (1 + K) = 384 roots)"""
    from bench_unsup_sage import build
    from euler_amd.models.sage_tower import UnsupSageTrainer

    monkeypatch.delenv("EULER_AMD_DW_ROUTE_WG", raising=False)
    tr = []
    for impl in (PIPE, BASE):
        monkeypatch.setenv("EULER_AMD_DW_ROUTE_IMPL", str(impl))
        graph, x, _ = build(6000, 30, 10, 32, 0.5, 7, cuda)
        graph.manual_seed(23)
        tr.append(UnsupSageTrainer(graph, 64, [10, 5], [64, 64, 32], features=x, num_negs=5, learning_rate=0.01,
                                   init_seed=7))
    a, b = tr
    assert a.pair is not None and b.pair is not None
    assert a.pair.splits() == b.pair.splits() and a.pair.folds() == b.pair.folds()
    a.forward_backward()
    b.forward_backward()
    _same(a.flat.grad, b.flat.grad, "grad")
    assert float(a.flat.grad.abs().sum()) > 0
    for _ in range(3):
        a.step()
        b.step()
    _same(a.flat.grad, b.flat.grad, "grad")
    _same(a.flat.flat, b.flat.flat, "flat")
    _same(a.opt.m, b.opt.m, "m")
    _same(a.opt.v, b.opt.v, "v")
    _same(a.loss_out, b.loss_out, "loss")
    for k in a._pair_keep:
        if "_sh" in k:
            _same(a._pair_keep[k], b._pair_keep[k], k)
    for t in a.towers:
        _same(a.towers[t]._keep["W0_sh"], b.towers[t]._keep["W0_sh"], t + ".W0_sh")
