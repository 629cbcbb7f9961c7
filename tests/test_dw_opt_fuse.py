"""The optimizer inside the dW launch (csrc/hip/tree_dw.hip tr_dw_all_kernel's trailing blocks
and tr_dw_fold_body's update; plan key ``dw_opt_fuse``).

Every case builds two trainers that differ only in ``dw_opt_fuse`` (1: the folded stored-G
problems update their tile in the block that summed it, and trailing blocks of the dW launch
reduce the routed slabs, wait for them per routed tile, and run the update; 0: the optimizer
launch of its own) on the same graph, weights and RNG counter, and asserts that the parameters,
the optimizer slots, the loss and every bf16 weight shadow are bitwise equal after three steps,
and that no wait of the fused launch timed out.  The shapes are the smallest at which the fused
launch takes another path: the routed problem's minimum of 8 slabs, routed splits past the last
k-block (zero slabs) with a short last slab, more workgroups than the device holds at once (the
trailing blocks queue behind their producers), two routed problems, the unsupervised pair step,
an optimizer other than Adam with weight decay, graph replays (the counters reset themselves),
back-to-back launches, and the plans that must keep the optimizer launch.
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


def _pair(monkeypatch, cuda, B, fanouts, dims, C, min_kps=None, D=32, route_wg=None, **kw):
    """two SageTrainers, dw_opt_fuse = 1 and 0, same graph / tables / weights / RNG counter"""
    from euler_amd.dataset.synthetic import synthetic_features, synthetic_labels
    from euler_amd.graph.device_graph import DeviceGraph
    from euler_amd.models.sage_trainer import SageTrainer

    for key, val in (("EULER_AMD_DW_MIN_KPS", min_kps), ("EULER_AMD_DW_ROUTE_WG", route_wg)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(val))
    monkeypatch.delenv("EULER_AMD_DW_FOLD", raising=False)
    feats = synthetic_features(N, D, 2, cuda)
    labels = synthetic_labels(feats, C)
    out = []
    for fuse in (1, 0):
        monkeypatch.setenv("EULER_AMD_DW_OPT_FUSE", str(fuse))
        g = DeviceGraph.synthetic(N, 8.0, 256, seed=1, device=cuda)
        g.manual_seed(23)
        out.append(SageTrainer(g, B, fanouts, dims, C, features=feats, labels=labels, learning_rate=1e-2,
                               init_seed=5, **kw))
    return out


def _compare(a, b):
    for name in ("flat", "m", "v", "loss_out", "counts"):
        _same(getattr(a, name), getattr(b, name), name)
    shadows = [k for k in a._buf if k.endswith("_sh") or k.endswith("_shT")]
    assert len(shadows) >= 5
    for k in shadows:
        _same(a._buf[k], b._buf[k], k)
    assert torch.isfinite(a.loss_out).all()
    assert a.fuse_error() == 0 and b.fuse_error() == 0


def _check_trainers(a, b, sync=None, fused=True):
    assert a.fused(sync) == fused and not b.fused(sync)
    assert a.plan.fused() == (fused or sync is not None) and not b.plan.fused()
    start = a.flat.clone()
    for _ in range(3):
        a.step(sync)
        b.step(sync)
    assert not torch.equal(start, a.flat)
    _compare(a, b)


@pytest.mark.gpu
def test_fold_minimum_eight_routed_slabs(cuda, monkeypatch):
    """the fold test's minimum shape with the routed problem at its minimum S = 8 (8 workgroups
    asked for; the other cases on this shape leave the default, S = 48), F = 3 in the folded ones"""
    a, b = _pair(monkeypatch, cuda, 96, [5, 3], [64, 64, 32], 5, min_kps=1, route_wg=8)
    assert a.plan.splits() == [8, 1, 1, 1] and a.plan.folds() == [0, 3, 3, 3]
    assert b.plan.splits() == a.plan.splits() and b.plan.folds() == a.plan.folds()
    _check_trainers(a, b)


@pytest.mark.gpu
def test_zero_slabs_and_a_short_last_slab(cuda, monkeypatch):
    """B = 160: 2560 target rows, MB = 80 k-blocks in S = 32 routed splits of kps = 3: splits
    0..25 are full, split 26 has 2 k-blocks, splits 27..31 lie past MB and write zero slabs"""
    a, b = _pair(monkeypatch, cuda, 160, [5, 3], [64, 64, 64], 40, min_kps=2, route_wg=32)
    assert a.M[1] == 2560 and a.plan.splits()[0] == 32 and a.plan.route_blocks(0) == 32
    _check_trainers(a, b)


@pytest.mark.gpu
def test_more_workgroups_than_the_device_holds(cuda, monkeypatch):
    """256 routed + 148 folded + 257 trailing workgroups at two per CU: the trailing blocks queue
    behind earlier blocks and every tile block starts late"""
    a, b = _pair(monkeypatch, cuda, 128, [5, 3], [256, 256, 64], 64, D=128)
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    assert a.plan.dw_blocks(True) == 256 + 148 + 257
    assert a.plan.dw_blocks(True) > 2 * cus, (a.plan.dw_blocks(True), cus)
    assert a.plan.splits()[0] == 32
    _check_trainers(a, b)


@pytest.mark.gpu
def test_three_hops_two_routed_problems(cuda, monkeypatch):
    a, b = _pair(monkeypatch, cuda, 64, [3, 2, 2], [64, 64, 64, 32], 8, min_kps=1, D=16)
    assert a.plan.folds() == [0, 0, 2, 2, 2] and len(a.plan.problems(True)) == 2
    _check_trainers(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["adagrad", "momentum"])
def test_other_optimizers_with_weight_decay(cuda, monkeypatch, opt):
    a, b = _pair(monkeypatch, cuda, 96, [5, 3], [64, 64, 32], 5, min_kps=1, optimizer=opt, weight_decay=1e-3)
    _check_trainers(a, b)


@pytest.mark.gpu
def test_graph_replays_against_eager_unfused_steps(cuda, monkeypatch):
    """capture(steps=4) runs 2 eager steps; three replays of the 4-step graph reuse the hand-off
    counters twelve times without a memset between them"""
    a, b = _pair(monkeypatch, cuda, 96, [5, 3], [64, 64, 32], 5, min_kps=1)
    assert a.fused() and not b.fused()
    a.capture(steps=4)
    for _ in range(3):
        a.replay_steps(4)
    for _ in range(2 + 12):
        b.step()
    torch.cuda.synchronize()
    _compare(a, b)


@pytest.mark.gpu
def test_back_to_back_launches(cuda, monkeypatch):
    """two fused launches with nothing between them (the second finds the counters the first
    reset) against dW, optimizer, dW, optimizer"""
    a, b = _pair(monkeypatch, cuda, 96, [5, 3], [64, 64, 32], 5, min_kps=1)
    a.step()
    b.step()
    pa, pb = a.plan, b.plan
    pa.dw(a._dw_all, None, True, 1.0)
    pa.dw(a._dw_all, None, True, 1.0)
    for _ in range(2):
        pb.dw(b._dw_all)
        pb.opt(2)
    _compare(a, b)
    with pytest.raises(RuntimeError):
        pb.dw(b._dw_all, None, True, 1.0)  # not a fused() plan
    with pytest.raises(RuntimeError):
        pa.dw(a._dw_all[:1], None, True, 1.0)  # not every problem


@pytest.mark.gpu
def test_unsupervised_pair_step(cuda, monkeypatch):
    from bench_unsup_sage import build
    from euler_amd.models.sage_tower import UnsupSageTrainer

    monkeypatch.delenv("EULER_AMD_DW_FOLD", raising=False)
    tr = []
    for fuse in (1, 0):
        monkeypatch.setenv("EULER_AMD_DW_OPT_FUSE", str(fuse))
        graph, x, _ = build(6000, 30, 10, 32, 0.5, 7, cuda)
        graph.manual_seed(23)
        tr.append(UnsupSageTrainer(graph, 64, [10, 5], [64, 64, 32], features=x, num_negs=5, learning_rate=0.01,
                                   init_seed=7))
    a, b = tr
    assert a.pair is not None and b.pair is not None
    assert a.pair.fused() and not b.pair.fused()
    assert a.pair.folds() == [0, 0, 1, 1, 3, 3]
    for _ in range(3):
        a.step()
        b.step()
    _same(a.flat.flat, b.flat.flat, "flat")
    _same(a.opt.m, b.opt.m, "m")
    _same(a.opt.v, b.opt.v, "v")
    _same(a.loss_out, b.loss_out, "loss")
    _same(a.mrr_sum, b.mrr_sum, "mrr_sum")
    assert torch.isfinite(a.loss_out).all()
    for k in a._pair_keep:
        if "_sh" in k:
            _same(a._pair_keep[k], b._pair_keep[k], k)
    for t in a.towers:
        _same(a.towers[t]._keep["W0_sh"], b.towers[t]._keep["W0_sh"], t + ".W0_sh")
    assert a.pair.fuse_error() == 0


@pytest.mark.gpu
def test_tower_plan_keeps_its_reduce_launch(cuda, monkeypatch):
    """the per-op tower step hands a gradient to torch's optimizer (a mode-0 reduce): the key is
    accepted, nothing is fused, the step is the same"""
    from bench_unsup_sage import build
    from euler_amd.models.sage_tower import UnsupSageTrainer

    tr = []
    for fuse in (1, 0):
        monkeypatch.setenv("EULER_AMD_DW_OPT_FUSE", str(fuse))
        graph, x, _ = build(6000, 30, 10, 32, 0.5, 7, cuda)
        graph.manual_seed(23)
        tr.append(UnsupSageTrainer(graph, 64, [10, 5], [64, 64, 32], features=x, num_negs=5, learning_rate=0.01,
                                   init_seed=7, fused=False))
    a, b = tr
    assert a.pair is None and b.pair is None
    for t in a.towers:
        assert not a.towers[t].plan.fused() and a.towers[t].plan.fuse_error() == 0
    for _ in range(3):
        a.step()
        b.step()
    _same(a.flat.flat, b.flat.flat, "flat")
    _same(a.loss_out, b.loss_out, "loss")
    for t in a.towers:
        _same(a.towers[t]._keep["W0_sh"], b.towers[t]._keep["W0_sh"], t + ".W0_sh")


@pytest.mark.gpu
def test_grad_sync_step_keeps_the_optimizer_launch(cuda, monkeypatch):
    a, b = _pair(monkeypatch, cuda, 96, [5, 3], [64, 64, 32], 5, min_kps=1)
    _check_trainers(a, b, sync=lambda g: 1.0, fused=False)
    _same(a.grad, b.grad, "grad")


@pytest.mark.gpu
def test_unfolded_problem_keeps_the_optimizer_launch(cuda, monkeypatch):
    """MB = 20 at one k-block per slab: 20 slabs > 16 stay in memory (F = 0), so the plan is not
    fused whatever the key says"""
    a, b = _pair(monkeypatch, cuda, 640, [5, 3], [64, 64, 64], 16, min_kps=1)
    assert a.plan.folds() == [0, 0, 0, 0] and a.plan.splits()[1:] == [20, 20, 20]
    assert not a.plan.fused() and not b.plan.fused()
    assert not a.fused() and not b.fused()
    for _ in range(3):
        a.step()
        b.step()
    _compare(a, b)
