"""The in-block split-K fold of the stored-G dW problems (csrc/hip/tree_dw.hip
tr_dw_fold_body; plan key ``dw_fold``).

Every case builds two trainers that differ only in ``dw_fold`` (1: the slabs of a 32x32 tile
are summed in the block's LDS and ``part`` holds one slab; 0: every slab goes through memory
and the optimizer launch sums them) on the same graph, weights and RNG counter, and asserts
that the gradient, the parameters, the optimizer slots, the loss and the bf16 weight shadows
are bitwise equal.  The shapes are the smallest at which the fold takes another path: a fold
count that is no multiple of the 4 waves, a short last slab, the headline's 4 k-blocks per
slab, more slabs than the LDS holds (the global path must stay), a 3-hop launch with two
routed problems beside the folded ones, the unsupervised pair step, and the two-bucket
data-parallel split whose dW launch holds no routed problem.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "benchmarks"))

N = 20_000


def _bits(t):
    return t.detach().reshape(-1).contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), f"{what}: {int((_bits(a) != _bits(b)).sum())} of {a.numel()} words differ"


def _pair(monkeypatch, cuda, B, fanouts, dims, C, min_kps=None, D=32, **kw):
    """two SageTrainers, dw_fold = 1 and 0, same graph / tables / weights / RNG counter"""
    from euler_amd.dataset.synthetic import synthetic_features, synthetic_labels
    from euler_amd.graph.device_graph import DeviceGraph
    from euler_amd.models.sage_trainer import SageTrainer

    if min_kps is None:
        monkeypatch.delenv("EULER_AMD_DW_MIN_KPS", raising=False)
    else:
        monkeypatch.setenv("EULER_AMD_DW_MIN_KPS", str(min_kps))
    feats = synthetic_features(N, D, 2, cuda)
    labels = synthetic_labels(feats, C)
    out = []
    for fold in (1, 0):
        monkeypatch.setenv("EULER_AMD_DW_FOLD", str(fold))
        g = DeviceGraph.synthetic(N, 8.0, 256, seed=1, device=cuda)
        g.manual_seed(23)
        out.append(SageTrainer(g, B, fanouts, dims, C, features=feats, labels=labels, learning_rate=1e-2,
                               init_seed=5, **kw))
    return out


def _check_trainers(a, b, sync=None):
    a.forward_backward()
    b.forward_backward()
    _same(a.grad, b.grad, "grad")
    assert float(a.grad.abs().sum()) > 0
    for _ in range(3):
        a.step(sync)
        b.step(sync)
    for name in ("flat", "m", "v", "loss_out", "grad"):
        _same(getattr(a, name), getattr(b, name), name)
    shadows = [k for k in a._buf if k.endswith("_sh") or k.endswith("_shT")]
    assert len(shadows) >= 5
    for k in shadows:
        _same(a._buf[k], b._buf[k], k)
    assert torch.isfinite(a.loss_out).all()


@pytest.mark.gpu
def test_fold_count_not_a_multiple_of_the_waves(cuda, monkeypatch):
    """MB = 3, one k-block per slab: F = 3, wave 3 of every block has no slab"""
    a, b = _pair(monkeypatch, cuda, 96, [5, 3], [64, 64, 32], 5, min_kps=1)
    assert a.plan.folds() == [0, 3, 3, 3] and a.plan.splits()[1:] == [1, 1, 1]
    assert b.plan.folds() == [0, 0, 0, 0] and b.plan.splits()[1:] == [3, 3, 3]
    assert a.plan.splits()[0] == b.plan.splits()[0]
    _check_trainers(a, b)


@pytest.mark.gpu
def test_short_last_slab(cuda, monkeypatch):
    """MB = 5, kps = 2: F = 3 and the last slab has one k-block"""
    a, b = _pair(monkeypatch, cuda, 160, [5, 3], [64, 64, 64], 40, min_kps=2)
    assert a.plan.folds() == [0, 3, 3, 3] and a.plan.splits()[1:] == [1, 1, 1]
    assert b.plan.folds() == [0, 0, 0, 0] and b.plan.splits()[1:] == [3, 3, 3]
    _check_trainers(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("buckets", [1, 2])
def test_two_slabs_of_four_k_blocks(cuda, monkeypatch, buckets):
    """MB = 8 at the default 4 k-blocks per slab (the headline's kps): F = 2.  buckets = 2:
    the data-parallel split, whose stored-G dW launch holds no routed problem"""
    a, b = _pair(monkeypatch, cuda, 256, [5, 3], [128, 128, 64], 64, grad_buckets=buckets)
    assert a.plan.folds() == [0, 2, 2, 2] and a.plan.splits()[1:] == [1, 1, 1]
    assert b.plan.folds() == [0, 0, 0, 0] and b.plan.splits()[1:] == [2, 2, 2]
    _check_trainers(a, b, (lambda g: 1.0) if buckets == 2 else None)


@pytest.mark.gpu
def test_more_slabs_than_the_lds_holds_keep_the_global_path(cuda, monkeypatch):
    """MB = 20, one k-block per slab: 20 slabs > 16, so fold count 0 and the old splits"""
    a, b = _pair(monkeypatch, cuda, 640, [5, 3], [64, 64, 64], 16, min_kps=1)
    assert a.plan.folds() == [0, 0, 0, 0] and a.plan.splits()[1:] == [20, 20, 20]
    assert a.plan.splits() == b.plan.splits() and b.plan.folds() == [0, 0, 0, 0]
    _check_trainers(a, b)


@pytest.mark.gpu
def test_three_hops_two_routed_problems_in_the_launch(cuda, monkeypatch):
    a, b = _pair(monkeypatch, cuda, 64, [3, 2, 2], [64, 64, 64, 32], 8, min_kps=1, D=16)
    assert a.plan.folds() == [0, 0, 2, 2, 2] and a.plan.splits()[2:] == [1, 1, 1]
    assert b.plan.folds() == [0, 0, 0, 0, 0] and b.plan.splits()[2:] == [2, 2, 2]
    assert a.plan.splits()[:2] == b.plan.splits()[:2]
    _check_trainers(a, b)


@pytest.mark.gpu
def test_unsupervised_pair_step(cuda, monkeypatch):
    """PairPlan plans W1 / Wfc of both towers with the same split plan: the source tower
    (B = 64 rows, MB = 2) has one slab, the context tower (B (1 + K) = 384 rows, MB = 12) three"""
    from bench_unsup_sage import build
    from euler_amd.models.sage_tower import UnsupSageTrainer

    tr = []
    for fold in (1, 0):
        monkeypatch.setenv("EULER_AMD_DW_FOLD", str(fold))
        graph, x, _ = build(6000, 30, 10, 32, 0.5, 7, cuda)
        graph.manual_seed(23)
        tr.append(UnsupSageTrainer(graph, 64, [10, 5], [64, 64, 32], features=x, num_negs=5, learning_rate=0.01,
                                   init_seed=7))
    a, b = tr
    assert a.pair is not None and b.pair is not None
    assert a.pair.folds() == [0, 0, 1, 1, 3, 3] and a.pair.splits()[2:] == [1, 1, 1, 1]
    assert b.pair.folds() == [0, 0, 0, 0, 0, 0] and b.pair.splits()[2:] == [1, 1, 3, 3]
    assert a.pair.splits()[:2] == b.pair.splits()[:2]
    a.forward_backward()
    b.forward_backward()
    _same(a.flat.grad, b.flat.grad, "grad")
    assert float(a.flat.grad.abs().sum()) > 0
    for _ in range(3):
        a.step()
        b.step()
    _same(a.flat.flat, b.flat.flat, "flat")
    _same(a.opt.m, b.opt.m, "m")
    _same(a.opt.v, b.opt.v, "v")
    _same(a.loss_out, b.loss_out, "loss")
    for k in a._pair_keep:
        if "_sh" in k:
            _same(a._pair_keep[k], b._pair_keep[k], k)
    for t in a.towers:
        _same(a.towers[t]._keep["W0_sh"], b.towers[t]._keep["W0_sh"], t + ".W0_sh")
