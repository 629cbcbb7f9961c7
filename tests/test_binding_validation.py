"""The operand-validation layer of the HIP bindings (csrc/hip/binding_util.h, docs/DESIGN.md 9j).

R1: every tensor operand is validated (GPU, the anchor's device, dtype, contiguity, element
count) before any allocation or launch; R3: a violation is a RuntimeError naming the op / plan
and the operand / dict key.

CPU: one row per exported free function (the table must equal the module's exports, so an op
cannot be added without a row); every row's well-typed CPU arguments raise without touching a
device; plan constructors name a missing key and refuse CPU tensors.
GPU: for a sample of ops from every binding file, each operand in turn is spoiled (wrong dtype,
CPU copy, non-contiguous view) and must be refused by name, the well-formed call giving the
same bits before and after; every plan class refuses a dict with one entry spoiled; with two
GPUs, one operand at a time on the other device.
"""
import pytest
import torch


def _m():
    from euler_amd.ops._native import hip

    return hip()


def f32(*s):
    return torch.zeros(*s, dtype=torch.float32)


def bf(*s):
    return torch.zeros(*s, dtype=torch.bfloat16)


def i32(*s):
    return torch.zeros(*s, dtype=torch.int32)


def i64(*s):
    return torch.zeros(*s, dtype=torch.int64)


def _csr():
    return i64(9), i32(4), f32(4)


def _upd():  # sgns_grad / sgns_apply_: ptr, list, coef, K, src, smap, sinv
    return i64(3), i32(2), f32(2, 2), 1, f32(4, 8), None, i64(4)


def _kg():  # ent, rel, src, dst, ridx, neg
    return f32(4, 8), f32(2, 8), i64(2), i64(2), i64(2), i64(2, 2)


_ADAM = (1e-3, 0.9, 0.999, 1e-8)

# name -> (builder of well-typed CPU arguments, the operand the op checks first: its anchor), or None for
# the functions that take no tensor operand
ROWS = {
    # binding.cpp
    "rng_advance": (lambda: (i64(2), 1), "rng_state"),
    "sample_neighbor": (lambda: (*_csr(), 8, 1, 1, i32(4), 2, -1, i64(2), 0, False), "nodes"),
    "alias_sample": (lambda: (f32(4), i32(4), None, 2, i64(2), 0), "prob"),
    "random_walk": (lambda: (*_csr(), 8, 1, i32(2), i32(4), -1, i64(2), 0), "starts"),
    "synth_csr": None,
    "sage_fwd": (lambda: (bf(8, 16), i32(4), i32(4, 2), bf(64, 32), None, True, True, False), "x"),
    "linear_fwd": (lambda: (bf(4, 32), bf(16, 32), None, False), "A"),
    "sage_bwd_scatter": (lambda: (bf(4, 32), i32(4), i32(4, 2), True, False, f32(8, 16)), "dA"),
    "relu_bwd_": (lambda: (bf(8), bf(8)), "grad"),
    "gather_rows": (lambda: (f32(16, 32), i64(16)), "x"),
    "gather_sum": (lambda: (f32(8, 4), i64(4, 2)), "x"),
    "segment_reduce": (lambda: (f32(4, 4), i64(3), None, 0, 0.0), "src"),
    "segment_reduce_wave": (lambda: (f32(4, 4), i64(3), None, 0), "src"),
    "index_add_rows_": (lambda: (f32(4, 4), i64(2), f32(2, 4)), "src"),
    "max_bwd": (lambda: (f32(2, 4), i64(2, 4), 4), "grad_out"),
    "edge_softmax": (lambda: (f32(4, 2), i64(3), None), "logits"),
    "edge_softmax_bwd": (lambda: (f32(4, 2), f32(4, 2), i64(3), None), "p"),
    "spmm_csr": (lambda: (i64(3), i64(4), None, f32(4, 4)), "x"),
    "flat_optim_": (lambda: (f32(8), f32(8), f32(8), f32(8), i64(1), *_ADAM, 0.0, 1.0, 0), "p"),
    "sparse_optim_": (lambda: (f32(4, 4), f32(4, 4), f32(4, 4), i64(2), f32(2, 4), i64(1), *_ADAM, 0), "table"),
    "sample_neighbor_into": (lambda: (*_csr(), 8, 1, 1, i32(4), 2, -1, i64(2), 0, i32(8)), "nodes"),
    # binding_gnn.cpp
    "route_by_owner": (lambda: (i64(4), 2, 4, i32(1)), "ids"),
    "gemm": (lambda: (f32(16, 32), f32(32, 16), f32(16, 16)), "A"),
    "gat_supported": None,
    "gat_fwd": (lambda: (i64(9), i32(8), None, f32(8, 32), f32(8, 4), f32(8, 4), 4, 8, 0.2), "h"),
    "gat_bwd": (lambda: (i64(9), i32(8), None, i64(9), i32(8), None, f32(8, 32), f32(8, 4), f32(8, 4), 4, 8, 0.2,
                         f32(8, 32), f32(8, 32), f32(8, 4)), "h"),
    "gat_att_fwd": (lambda: (f32(8, 32), f32(4, 8), f32(4, 8), 4, 8), "z"),
    "gat_att_bwd_": (lambda: (f32(8, 32), f32(4, 8), f32(4, 8), 4, 8, f32(8, 4), f32(8, 4), f32(8, 32)), "z"),
    "rel_gemm": (lambda: (bf(4, 32), i32(4), i32(1), i32(1), i32(1), bf(1, 16, 32), None, i32(4), 0, 16, bf(4, 16)),
                 "A"),
    "rel_gemm_dw": (lambda: (bf(4, 64), i32(4), bf(4, 64), i32(4), None, i32(1), i32(1), i32(1), None,
                             f32(1, 64, 64)), "G"),
    "rel_weight_bf16": (lambda: (f32(1, 64, 64),), "W"),
    "sgns_fwd": (lambda: (f32(2, 8), f32(2, 1, 8), f32(2, 2, 8)), "emb"),
    "sgns_bwd": (lambda: (f32(2, 8), f32(2, 1, 8), f32(2, 2, 8), f32(2, 3), 1.0), "emb"),
    "sgns_fwd_idx": (lambda: (f32(4, 8), None, i64(2), f32(4, 8), None, i64(4), 1, 1.0), "T"),
    "occ_csr": (lambda: (i64(4), 2), "inv"),
    "sgns_grad": (lambda: (0, *_upd(), None), "src"),
    "gather_f32_bf16": (lambda: (f32(4, 8), i64(2)), "x"),
    "sgns_apply_": (lambda: (0, *_upd(), f32(4, 8), f32(4, 8), f32(4, 8), None, i64(1), True, *_ADAM, 0), "src"),
    "kg_fwd": (lambda: (*_kg(), 0, 0, False), "ent"),
    "kg_step": (lambda: (f32(4, 8), f32(2, 8), i64(2), i64(2), i64(2), i64(2), i64(1), 0, 0, False, 1.0, i64(2),
                         i64(2), i64(2), i64(2, 2), f32(2), f32(4), f32(1), f32(4, 8), f32(2, 8)), "h"),
    "det_occ": (lambda: (i64(4), 2), "keys"),
    "det_segment_sum": (lambda: (f32(4, 4), i64(3), i32(4), f32(2, 4)), "src"),
    "kg_step_parts": None,
    "cast_bf16": (lambda: (f32(8), bf(8)), "x"),
    "drop_rows": (lambda: (f32(2, 4), 0.5, 0, i64(1), 0, f32(2, 4), f32(2)), "x"),
    "zero_": (lambda: (f32(4),), "t"),
    "memset_zero": (lambda: (f32(4),), "t"),
    "graph_summary": None,
    "graph_upload": None,
    "seg_count": (lambda: (i64(4), 2), "idx"),
    "flow_block": (lambda: (i64(4), i64(2), i64(6), i64(6), i64(1), i64(2), i64(1), 4, False, i32(1)), "src"),
    "gcn_norm_weight": (lambda: (i64(2, 4), i64(4), i64(4)), "edge_index"),
    "sage_block": (lambda: (i64(6), i64(6), i64(1), i64(2), 2, 4, False), "inv"),
    "bce_f1_fwd": (lambda: (f32(2, 4), f32(8, 4), i64(2), i64(3)), "x"),
    "bce_bwd": (lambda: (f32(2, 4), f32(8, 4), i64(2), f32(1)), "x"),
    "pair_fwd": (lambda: (f32(2, 8), f32(4, 8), 2, 1), "es"),
    "pair_bwd": (lambda: (f32(2, 8), f32(4, 8), 2, 1, f32(2, 2), f32(1), f32(2, 8), f32(4, 8)), "es"),
    "kg_bwd": (lambda: (*_kg(), 0, 0, False, f32(2), f32(2, 2), f32(4, 8), f32(2, 8)), "ent"),
    "unique_first": (lambda: (i64(4),), "x"),
    "unique_first_padded": (lambda: (i64(4),), "x"),
    "full_neighbors": (lambda: (i64(9), i32(4), 8, 1, 1, i64(2), 8, i32(1)), "rows"),
    # binding_knn.cpp
    "knn_flat_scan": (lambda: (f32(4, 8), f32(16, 8), f32(16), 2, 1), "q"),
    "knn_ivf_scan": (lambda: (f32(4, 8), f32(16, 8), f32(16), i64(3), i64(16), i64(4, 1), 2), "q"),
    "knn_merge": (lambda: (f32(4, 1, 2), i64(4, 1, 2), f32(4)), "dist"),
    # binding_kg_rank.cpp
    "kg_rank_counts": (lambda: (f32(4, 8), f32(16, 8), i64(4), 1), "q"),
    # binding_sage_csr.cpp
    "sage_csr_fwd": (lambda: (*_csr(), 1, 1, bf(8, 16), bf(64, 32)), "x"),
    # binding_graph_build.cpp
    "graph_build_pack": (lambda: (i64(4), i64(4), None, None, None, 8, 1, 3, False, i64(4)), "src"),
    "graph_build_sort": (lambda: (i64(4), i32(4), 3), "keys"),
    "graph_build_heads": (lambda: (i64(4), i64(4)), "keys"),
    "graph_build_compact": (lambda: (i64(4), i32(4), i32(4), None, 4, 2), "keys"),
    "graph_build_csr": (lambda: (i64(4), i32(4), None, 4, 8, 1, 3), "keys"),
    # binding_node_embed.cpp
    "node_bag_fwd": (lambda: (i64(4), None, None, None, f32(8, 4), f32(4, 4), 0, 2, False), "table"),
    "node_bag_bwd_": (lambda: (f32(8, 4), i64(4), None, None, None, f32(4, 4), 0, 2, False), "dtable"),
    # binding_walk_shard.cpp
    "walk_keys": (lambda: (i32(4), i32(4, 3), 8, 8, 1, 0), "starts"),
    "walk_step_owner": (lambda: (i64(4), 8, 1, *_csr(), 8, 1, 1, 0, i64(2), 0), "req"),
    "walk_unroute": (lambda: (i32(4), i64(4), i32(4, 3), 1, 0, 8, 8, 1, 0), "back"),
}
PLANS = {"TreePlan", "TowerPlan", "PairPlan", "GcnPlan", "GraphClsPlan"}
CLASSES = PLANS | {"XgmiAr"}
CHECKED = sorted(n for n, r in ROWS.items() if r is not None)


def _named(msg, op, operand):
    """R3: the message names the op / plan and the operand / key"""
    return op in msg and (f": {operand} " in msg or f"'{operand}'" in msg)


# ----------------------------------------------------------------------------------------- CPU


def test_table_covers_every_export():
    m = _m()
    exported = {n for n in dir(m) if not n.startswith("_") and callable(getattr(m, n))}
    assert set(ROWS) | CLASSES == exported
    assert not set(ROWS) & CLASSES
    assert len(ROWS) == 76 and sum(r is None for r in ROWS.values()) == 5


@pytest.mark.parametrize("name", CHECKED)
def test_cpu_operands_are_refused_by_name(name):
    build, first = ROWS[name]
    with pytest.raises(RuntimeError) as e:
        getattr(_m(), name)(*build())
    assert _named(str(e.value), name, first), str(e.value)


def _cpu_plan_dicts():
    graph = {"indptr": i64(9), "rng": i64(2), "nbr": i32(4), "cumw": f32(4), "num_types": 1}
    return {
        "TreePlan": ({"L": 1, "B": 32, "F": [0, 2], "logP": [0], "masks": [0, 1], "H": [64], "D": 16, "E": 32,
                      "C": 32, "C_real": 4, "include_self": 1, **graph}, "B", "indptr"),
        "TowerPlan": ({"R": 32, "F1": 2, "F2": 2, "logP": 4, "D": 16, "H": 64, "include_self": 1, "mask1": 1,
                       **graph}, "R", "indptr"),
        "GcnPlan": ({"L": 1, "B": 4, "self_loops": 1, **graph}, "L", "indptr"),
        "GraphClsPlan": ({"L": 1, "B": 2, "kind": 0, "self_loops": 0, "nmax": 16, "E": 16, "C": 2, "G": 2,
                          "tab_rows": 1, "D": [16, 16], "adj_pair": [i32(4)], "adj_of": [0], "rec": i32(16)},
                         "nmax", "rec"),
    }


# PairPlan takes two constructed TowerPlans, which need a GPU: it is covered in the GPU part
@pytest.mark.parametrize("plan", sorted(PLANS - {"PairPlan"}))
def test_plan_constructors_name_missing_keys_and_refuse_cpu_tensors(plan):
    d, scalar, tensor = _cpu_plan_dicts()[plan]
    ctor = getattr(_m(), plan)
    with pytest.raises(RuntimeError) as e:
        ctor(dict(d))
    assert _named(str(e.value), plan, tensor) and "GPU" in str(e.value), str(e.value)
    for key in (scalar, tensor):
        with pytest.raises(RuntimeError) as e:
            ctor({k: v for k, v in d.items() if k != key})
        assert _named(str(e.value), plan, key) and "missing" in str(e.value), str(e.value)


# ----------------------------------------------------------------------------------------- GPU
# one well-formed call per binding file that exports free functions: (op, file, operands by
# the name the binding gives them, call).  Smallest shapes only.


def _ring(dev, n=8, deg=2):
    """CSR of a ring: row i -> i+1 .. i+deg (one edge type), cumulative weights per row"""
    indptr = torch.arange(0, (n + 1) * deg, deg, dtype=torch.int64, device=dev)
    nbr = ((torch.arange(n * deg, device=dev) // deg + torch.arange(n * deg, device=dev) % deg + 1) % n).int()
    cumw = (torch.arange(n * deg, device=dev) % deg + 1).float()
    return indptr, nbr, cumw


def _samples(dev):
    g = torch.Generator().manual_seed(11)

    def rnd(*s, dt=torch.float32):
        return torch.randn(*s, generator=g).to(dev).to(dt)

    indptr, nbr, cumw = _ring(dev)
    x = rnd(16, 8)
    wide = rnd(16, 64)
    return [
        ("knn_flat_scan", "binding_knn.cpp", {"q": rnd(4, 8), "x": x, "xn": (x * x).sum(1)},
         lambda m, o: m.knn_flat_scan(o["q"], o["x"], o["xn"], 2, 1)),
        ("gather_rows", "binding.cpp", {"x": rnd(16, 32), "idx": torch.arange(15, -1, -1, device=dev)},
         lambda m, o: [m.gather_rows(o["x"], o["idx"])]),
        ("sample_neighbor", "binding.cpp",
         {"indptr": indptr, "nbr": nbr, "cumw": cumw, "nodes": torch.arange(8, device=dev).int(),
          "rng_state": torch.tensor([3, 0], device=dev)},
         lambda m, o: m.sample_neighbor(o["indptr"], o["nbr"], o["cumw"], 8, 1, 1, o["nodes"], 2, -1,
                                        o["rng_state"], 0, False)),
        ("gemm", "binding_gnn.cpp", {"A": rnd(16, 32), "B": rnd(32, 16), "C": torch.zeros(16, 16, device=dev)},
         lambda m, o: [m.gemm(o["A"], o["B"], o["C"]), o["C"].clone()][1:]),
        # the documented exception to contiguity: a row stride that is not the width
        ("gemm", "binding_gnn.cpp", {"A": wide[:, :32], "B": rnd(32, 16), "C": torch.zeros(16, 16, device=dev)},
         lambda m, o: [m.gemm(o["A"], o["B"], o["C"]), o["C"].clone()][1:]),
        ("gat_fwd", "binding_gnn.cpp",
         {"indptr": indptr, "col": nbr, "h": rnd(8, 32), "al": rnd(8, 4), "ar": rnd(8, 4)},
         lambda m, o: m.gat_fwd(o["indptr"], o["col"], None, o["h"], o["al"], o["ar"], 4, 8, 0.2)),
        ("kg_rank_counts", "binding_kg_rank.cpp",
         {"q": rnd(4, 8), "cands": rnd(16, 8), "true_idx": torch.tensor([0, 5, 9, 15], device=dev)},
         lambda m, o: m.kg_rank_counts(o["q"], o["cands"], o["true_idx"], 1)),
        ("sage_csr_fwd", "binding_sage_csr.cpp",
         {"indptr": indptr, "nbr": nbr, "cumw": cumw, "x": rnd(8, 16, dt=torch.bfloat16),
          "W": rnd(64, 32, dt=torch.bfloat16)},
         lambda m, o: [m.sage_csr_fwd(o["indptr"], o["nbr"], o["cumw"], 1, 1, o["x"], o["W"])]),
        ("graph_build_heads", "binding_graph_build.cpp",
         {"keys": torch.arange(16, device=dev) // 2, "status": torch.zeros(4, dtype=torch.int64, device=dev)},
         lambda m, o: [m.graph_build_heads(o["keys"], o["status"])]),
        ("node_bag_fwd", "binding_node_embed.cpp",
         {"rows": torch.tensor([1, 0, 7, 3], device=dev), "table": rnd(8, 4), "out": torch.zeros(4, 4, device=dev)},
         lambda m, o: [m.node_bag_fwd(o["rows"], None, None, None, o["table"], o["out"], 0, 2, False),
                       o["out"].clone()][1:]),
        ("walk_keys", "binding_walk_shard.cpp",
         {"starts": torch.tensor([1, 0, 7, 3], device=dev).int(),
          "out": torch.zeros(4, 3, dtype=torch.int32, device=dev)},
         lambda m, o: [m.walk_keys(o["starts"], o["out"], 8, 8, 1, 0), o["out"].clone()]),
    ]


# operands an op takes in any dtype (gather_rows copies whole rows): no dtype to get wrong
ANY_DTYPE = {("gather_rows", "x")}


def _wrong_dtype(t):
    """a dtype no op takes in that place: float64 (float16 for a float64 operand), int16"""
    if t.is_floating_point():
        return t.to(torch.float16 if t.dtype == torch.float64 else torch.float64)
    return t.to(torch.int16)


def _strided(t):
    """the same values as every second element of a buffer twice as long"""
    buf = torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)
    v = buf[::2].view(t.shape)
    v.copy_(t)
    assert not v.is_contiguous()
    return v


def _refused(call, m, ops, name, bad, op):
    with pytest.raises(RuntimeError) as e:
        call(m, {**ops, name: bad})
    assert _named(str(e.value), op, name), str(e.value)


def test_samples_cover_every_binding_file_with_free_functions():
    files = {s[1] for s in _samples("cpu")}
    # binding_tree.cpp, binding_gcn.cpp and binding_graph_cls.cpp export plan classes only
    assert files == {"binding.cpp", "binding_gnn.cpp", "binding_knn.cpp", "binding_kg_rank.cpp",
                     "binding_sage_csr.cpp", "binding_graph_build.cpp", "binding_node_embed.cpp",
                     "binding_walk_shard.cpp"}


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(11))
def test_each_operand_spoiled_is_refused_and_the_op_still_gives_the_same_bits(cuda, k):
    m = _m()
    op, _, ops, call = _samples(cuda)[k]
    before = [t.clone() for t in call(m, ops)]
    for name, t in ops.items():
        if (op, name) not in ANY_DTYPE:
            _refused(call, m, ops, name, _wrong_dtype(t), op)
        _refused(call, m, ops, name, t.cpu(), op)
        _refused(call, m, ops, name, _strided(t), op)
    after = call(m, ops)
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after))


# ---- plan classes: the smallest trainers of the existing suites; keys -> whether the plan
# checks an exact element count for them


def _spoil_plan(ctor, d, plan, keys):
    for key, sized in keys.items():
        t = d[key]
        bad = [_wrong_dtype(t), t.cpu(), None]
        if sized:
            bad.append(torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device))
        for b in bad:
            with pytest.raises(RuntimeError) as e:
                ctor({**d, key: b})
            assert _named(str(e.value), plan, key), (key, str(e.value))
    ctor(dict(d))  # the untouched dict still constructs


@pytest.fixture(scope="module")
def sage(cuda):
    from test_sage_trainer import _trainer

    return _trainer(cuda, [2, 2], [64, 64, 32], 10, B=32)


@pytest.fixture(scope="module")
def unsup(cuda):
    from test_unsup_sage import _setup

    return _setup("cuda", n=2000, comm=10, dims=(64, 64, 32), B=32, fan=(2, 2), K=1)[0]


@pytest.mark.gpu
def test_tree_plan_refuses_a_spoiled_dict(sage):
    keys = {"indptr": False, "nbr": False, "cumw": True, "node_prob": False, "node_alias": True, "rng": True,
            "features": False, "roots": True, "nodes": True, "leaf": True, "step": True, "W0_sh": True, "A0_kt": True,
            "mask0": True, "A1": True, "flat": False, "grad": True, "m": True, "v": True, "bfc": True,
            "loss_out": True, "counts": True}
    _spoil_plan(_m().TreePlan, sage._buf, "TreePlan", keys)


@pytest.mark.gpu
def test_tower_and_pair_plans_refuse_a_spoiled_dict(unsup):
    tower = unsup.towers["gnn"]
    keys = {"indptr": False, "nbr": False, "cumw": True, "node_prob": False, "node_alias": True, "rng": True,
            "roots_in": True, "nodes": True, "leaf": True, "features": False, "W0_sh": True, "A0_kt": True,
            "mask0": True, "A1": True, "dA1": True, "W0": True, "gW0": True}
    _spoil_plan(_m().TowerPlan, tower._keep, "TowerPlan", keys)
    s, c = unsup.towers["gnn"].plan, unsup.towers["context_gnn"].plan
    keys = {"step": True, "flat": False, "grad": True, "m": True, "v": True, "loss_acc": True, "loss_out": True,
            "mrr_sum": True, "W1_sh_s": True, "Wfc_shT_c": True, "bfc_c": True}
    _spoil_plan(lambda d: _m().PairPlan(s, c, d), unsup._pair_keep, "PairPlan", keys)


@pytest.mark.gpu
def test_gcn_plan_refuses_a_spoiled_dict(cuda):
    from euler_amd.models.gcn_trainer import GcnTrainer
    from test_gcn_trainer import _graph, _materialize, _setup

    m = _setup("cuda", layers=1, batch=32)
    g = _graph(m, cuda)
    _materialize(m, g, 32)
    tr = GcnTrainer.from_model(m, g, 32, caps="exact")
    keys = {"indptr": False, "nbr": False, "node_prob": False, "node_alias": True, "rng": True, "overflow": True,
            "features": False, "labels": True, "w0": True, "g_w0": True, "wfc": True, "bfc": True, "wout": True,
            "g_wout": True, "loss_out": True, "counts": True}
    _spoil_plan(_m().GcnPlan, tr._buf, "GcnPlan", keys)


@pytest.mark.gpu
def test_graph_cls_plan_refuses_a_spoiled_dict(tmp_path):
    from test_graph_cls_trainer import _est, _trainer

    tr = _trainer(_est(tmp_path, "gin", "cuda")[1])
    keys = {"rec": True, "gprob": True, "galias": True, "rng": True, "fpair": False, "fw": True, "onehot": True,
            "table": True, "Wfc": True, "bfc": True, "Wout": True, "warm": False, "grad": False, "loss_out": True,
            "right": True}
    _spoil_plan(_m().GraphClsPlan, tr._plan_dict(), "GraphClsPlan", keys)


# ---- cross-device cases last: with R1 in place none of them launches a kernel


def _two_gpus():
    return torch.cuda.is_available() and torch.cuda.device_count() >= 2


def _cross(call, m, ops, name, op):
    with pytest.raises(RuntimeError) as e:
        call(m, {**ops, name: ops[name].to("cuda:1")})
    assert _named(str(e.value), op, name) and "cuda:1" in str(e.value), str(e.value)


@pytest.mark.gpu
@pytest.mark.skipif(not _two_gpus(), reason="needs two GPUs")
def test_device_mismatch_regressions(cuda):
    """both passed validation before the shared layer and reached the kernel"""
    m = _m()
    by_op = {s[0]: s for s in _samples(cuda)}
    op, _, ops, call = by_op["sample_neighbor"]
    _cross(call, m, ops, "indptr", op)  # indptr on cuda:1, nodes (the anchor) on cuda:0
    op, _, ops, call = by_op["gat_fwd"]
    _cross(call, m, ops, "al", op)  # al on cuda:1, h (the anchor) on cuda:0


@pytest.mark.gpu
@pytest.mark.skipif(not _two_gpus(), reason="needs two GPUs")
def test_one_operand_on_the_other_gpu_is_refused(cuda, sage):
    m = _m()
    for op, _, ops, call in _samples(cuda):
        for name in ops:
            with pytest.raises(RuntimeError) as e:
                call(m, {**ops, name: ops[name].to("cuda:1")})
            assert op in str(e.value), (op, name, str(e.value))
    for key in ("indptr", "features", "flat", "labels"):
        with pytest.raises(RuntimeError) as e:
            m.TreePlan({**sage._buf, key: sage._buf[key].to("cuda:1")})
        assert "TreePlan" in str(e.value), (key, str(e.value))


@pytest.mark.gpu
@pytest.mark.skipif(not _two_gpus(), reason="needs two GPUs")
def test_xgmi_run_never_launches_on_the_current_device(cuda):
    """an all-reduce object of cuda:0 with cuda:1 current: a tensor of the current device is
    refused by name, and a tensor of its own device gets as far as the peers check (no launch
    either way)"""
    ar = _m().XgmiAr(1024)
    with torch.cuda.device(1):
        with pytest.raises(RuntimeError) as e:
            ar.run(torch.zeros(64, device="cuda:1"), 1)
        assert _named(str(e.value), "XgmiAr.run", "tensor") and "cuda:1" in str(e.value), str(e.value)
        with pytest.raises(RuntimeError, match="open"):
            ar.run(torch.zeros(64, device="cuda:0"), 1)
