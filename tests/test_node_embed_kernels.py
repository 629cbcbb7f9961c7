"""The node-row embedding-bag kernels (csrc/hip/node_embed.hip, ops/mp_ops.py ``node_bag``)
and the device-path trainers over sparse-feature / id inputs, on the GPU.

Kernel tests: tables and output gradients are dyadic (multiples of 1/8, magnitude <= 8), so
every sum here (fewer than 2^15 terms of at most 2^3 with 3 fractional bits) and every
``1 / count`` of the mean (power-of-two counts) is exact in fp32 in any order: forward and
backward are compared with ``torch.equal`` against the pure-torch CPU twin.  Shapes are the
smallest that reach every branch: V = 37, n = 67 (more than one group stride), D = 16
(4 lanes per bag), 128 (32 lanes per bag) and 20 (one lane per column), bag lengths that
are 0, below / equal to / above the unroll of 4 and up to 80, rows with -1, duplicates and
one past the table, ids that are negative, >= V and >= 2^33."""
import logging
import math
import re

import numpy as np
import pytest
import torch

V, N_OUT, N_ROWS = 37, 67, 29
SENTINEL = -777.0


def _dyadic(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-64, 65, shape, generator=g).float() / 8.0


def _inputs(mean=False, n=N_OUT, seed=0):
    """(rows [n], (indptr [N_ROWS + 1], values), node ids [N_ROWS]) on the CPU"""
    g = torch.Generator().manual_seed(seed)
    choices = [0, 1, 2, 4, 8, 64] + ([] if mean else [80])
    lens = torch.tensor([choices[i % len(choices)] for i in range(N_ROWS)])
    lens = lens[torch.randperm(N_ROWS, generator=g)]
    indptr = torch.zeros(N_ROWS + 1, dtype=torch.long)
    indptr[1:] = torch.cumsum(lens, 0)
    nnz = int(indptr[-1])
    values = torch.randint(0, V, (nnz,), generator=g)
    odd = torch.randperm(nnz, generator=g)[:24]
    values[odd[:8]] = -torch.randint(1, 1 << 40, (8,), generator=g)          # negative ids
    values[odd[8:16]] = V + torch.randint(0, 1000, (8,), generator=g)          # >= V
    values[odd[16:]] = (1 << 33) + torch.randint(0, 1 << 40, (8,), generator=g)  # >= 2^33
    rows = torch.randint(0, N_ROWS, (n,), generator=g)
    if n >= 8:
        rows[1] = rows[5] = rows[0]          # duplicates
        rows[2] = rows[n - 1] = -1           # the default node / padding
        rows[3] = N_ROWS                     # past the table: the default id
        rows[4] = int(torch.nonzero(lens == 0)[0])  # an empty bag
    ids = torch.sort(torch.randperm(3 * V, generator=g)[:N_ROWS]).values  # sorted, non-contiguous, some >= V
    return rows, (indptr, values), ids


def _index(mode, csr, ids, id_column=True):
    return (ids if id_column else None) if mode == "id" else csr


def _dev(x, device):
    if x is None:
        return None
    return tuple(t.to(device) for t in x) if isinstance(x, tuple) else x.to(device)


def _forward_case(device, D, mode, hash, n=N_OUT, id_column=True):
    from euler_amd.ops.mp_ops import node_bag

    rows, csr, ids = _inputs(mean=mode == "bag_mean", n=n)
    ix = _index(mode, csr, ids, id_column)
    table = _dyadic((V, D), 7)
    col, ld = 5, D + 9
    want = node_bag(table, rows, ix, mode, hash)
    buf = torch.full((n, ld), SENTINEL, device=device)
    got = node_bag(table.to(device), rows.to(device), _dev(ix, device), mode, hash, out=buf, col=col)
    assert got.data_ptr() == buf.data_ptr()
    res = buf.cpu()
    assert torch.equal(res[:, col: col + D], want)
    assert bool((res[:, :col] == SENTINEL).all()) and bool((res[:, col + D:] == SENTINEL).all())
    plain = node_bag(table.to(device), rows.to(device), _dev(ix, device), mode, hash)
    assert plain.shape == (n, D) and torch.equal(plain.cpu(), want)
    return want


def _backward_case(device, D, mode, hash, zero_padded=False, n=N_OUT):
    from euler_amd.ops.mp_ops import node_bag

    rows, csr, ids = _inputs(mean=mode == "bag_mean", n=n)
    ix = _index(mode, csr, ids)
    col, ld = 5, D + 9
    dout = _dyadic((n, ld), 11)
    if zero_padded:
        dout[rows < 0] = 0.0
    grads = []
    for dev in ("cpu", device):
        table = _dyadic((V, D), 7).to(dev).requires_grad_(True)
        buf = torch.full((n, ld), SENTINEL, device=dev)
        out = node_bag(table, rows.to(dev), _dev(ix, dev), mode, hash, out=buf, col=col)
        out.backward(dout.to(dev))  # autograd: fills table.grad
        assert table.grad is not None and table.grad.shape == (V, D)
        grads.append(table.grad.cpu())
    assert torch.equal(grads[1], grads[0])
    return rows, csr, dout, grads[1]


# ----------------------------------------------------------------------------- 7. forward
@pytest.mark.gpu
@pytest.mark.parametrize("hash", [False, True])
@pytest.mark.parametrize("mode", ["bag_sum", "bag_mean", "id"])
@pytest.mark.parametrize("D", [16, 20, 128])
def test_node_bag_forward_matches_twin(D, mode, hash):
    want = _forward_case("cuda", D, mode, hash)
    assert bool(want.abs().sum() > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bag_sum", "id"])
def test_node_bag_empty_input_launches_nothing(mode):
    from euler_amd.ops.mp_ops import node_bag

    _forward_case("cuda", 16, mode, False, n=0)
    rows, csr, ids = _inputs(n=0)
    table = _dyadic((V, 16), 7).cuda().requires_grad_(True)
    out = node_bag(table, rows.cuda(), _dev(_index(mode, csr, ids), "cuda"), mode, False)
    out.sum().backward()
    assert out.shape == (0, 16) and bool((table.grad == 0).all())


def test_node_bag_twin_semantics_cpu():
    """the CPU twin against a per-row loop of the documented rules (the twin is the GPU
    tests' reference): default id for empty bags / negative rows / rows past the table,
    clamp or hash of every id, CSR-order sum, mean = sum * (1 / count)"""
    from euler_amd.ops.mp_ops import node_bag

    table = _dyadic((V, 20), 7)
    for mode in ("bag_sum", "bag_mean", "id"):
        for hash in (False, True):
            rows, (indptr, values), ids = _inputs(mean=mode == "bag_mean")

            def row_of(v):
                if hash:
                    return ((v * 0x9E3779B1) % (1 << 64) & 0x7FFFFFFF) % V
                return v if 0 <= v < V else V - 1

            want = torch.zeros(rows.numel(), 20)
            for i, r in enumerate(rows.tolist()):
                inside = 0 <= r < N_ROWS
                if mode == "id":
                    bag = [int(ids[r])] if inside else [V - 1]
                else:
                    bag = values[int(indptr[r]): int(indptr[r + 1])].tolist() if inside else []
                    bag = bag or [V - 1]
                acc = torch.zeros(20)
                for v in bag:
                    acc = acc + table[row_of(v)]
                want[i] = acc * (1.0 / len(bag)) if mode == "bag_mean" else acc
            got = node_bag(table, rows, ids if mode == "id" else (indptr, values), mode, hash)
            assert torch.equal(got, want), (mode, hash)


# ----------------------------------------------------------------------------- 8. backward
@pytest.mark.gpu
@pytest.mark.parametrize("hash", [False, True])
@pytest.mark.parametrize("mode", ["bag_sum", "bag_mean", "id"])
@pytest.mark.parametrize("D", [16, 20, 128])
def test_node_bag_backward_matches_twin(D, mode, hash):
    _backward_case("cuda", D, mode, hash)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bag_sum", "bag_mean"])
def test_node_bag_backward_padded_rows_with_zero_gradient(mode):
    """the -1 rows carry a zero output gradient (a capacity-padded hop set): row V - 1 gets
    exactly what the real rows send it (their default-id bags and their ids >= V)"""
    D = 16
    rows, (indptr, values), dout, grad = _backward_case("cuda", D, mode, False, zero_padded=True)
    want = torch.zeros(D)
    for i, r in enumerate(rows.tolist()):
        if r < 0:
            continue
        bag = values[int(indptr[r]): int(indptr[r + 1])].tolist() if r < N_ROWS else []
        bag = bag or [V - 1]
        hits = sum(1 for v in bag if not 0 <= v < V - 1)
        scale = 1.0 / len(bag) if mode == "bag_mean" else 1.0
        want += dout[i, 5: 5 + D] * scale * hits
    assert torch.equal(grad[V - 1], want)


# ----------------------------------------------------------------------------- 9. id mode
@pytest.mark.gpu
@pytest.mark.parametrize("hash", [False, True])
@pytest.mark.parametrize("id_column", [False, True])
def test_node_bag_id_mode_with_and_without_id_column(id_column, hash):
    from euler_amd.ops.mp_ops import node_bag

    _check_id_mode("cuda", id_column, hash)


def _check_id_mode(device, id_column, hash):
    from euler_amd.ops.mp_ops import node_bag

    want = _forward_case(device, 16, "id", hash, id_column=id_column)
    rows, _, ids = _inputs()
    table = _dyadic((V, 16), 7)
    default = torch.tensor(V - 1)
    if id_column:  # sorted non-contiguous ids; a row past the column is the default id
        raw = torch.where((rows >= 0) & (rows < N_ROWS), ids[rows.clamp(0, N_ROWS - 1)], default)
    else:          # ids = rows
        raw = torch.where(rows >= 0, rows, default)
    tr = ((raw * 0x9E3779B1) & 0x7FFFFFFF) % V if hash else torch.where((raw < 0) | (raw >= V), default, raw)
    assert torch.equal(want, table[tr])
    assert torch.equal(node_bag(table, rows, ids if id_column else None, "id", hash), want)


# ----------------------------------------------------------------------------- trainers
@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("cora_sparse"))


def _setup(device, data_dir, batch=64, flags=("--use_sparse_feature", "--use_id")):
    """(model, estimator, device graph with fp32 features) of GeniePath on cora_sparse"""
    from euler_amd.graph.device_graph import DeviceGraph
    from euler_amd.tools import runner

    a = runner.parse_args(["--dataset", "cora_sparse", "--scale", "0.05", "--batch_size", str(batch), "--device",
                           device, "--seed", "1", "--data_dir", data_dir] + list(flags), model="geniepath")
    torch.manual_seed(0)
    m, est = runner.build(a)
    est._prepare(est.get_train_from_input(batch, est.params))
    ne = m._encoder._node_encoder
    g = DeviceGraph.from_engine(features=ne.feature_idx, feature_dims=ne.feature_dim, label=m.label_idx,
                                label_dim=m.label_dim, feature_dtype=torch.float32,
                                sparse_features=ne.sparse_feature_idx, seed=5, device=device)
    return m, est, g


def _step_vs_cpu_oracle(device, data_dir):
    import euler_amd.ops.graph_api as ge
    import torch.nn.functional as F
    from euler_amd.models.encoder_trainer import EncoderFlowTrainer

    m, est, g = _setup(device, data_dir)
    ne = m._encoder._node_encoder
    with torch.no_grad():  # the sparse tables start at std 2e-4: make their part of the input count
        for t in [ne.embedding] + list(ne.sparse_embeddings):
            t.weight.normal_(0.0, 0.1)
    tr = EncoderFlowTrainer.from_model(m, g, 64, learning_rate=0.01)
    loss = tr._forward_loss()
    tr.opt.zero_grad()
    loss.backward()
    grads = {n: p.grad.detach().float().cpu().clone() for n, p in m.named_parameters()}
    roots = tr._samples.cpu()
    state = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    # fp32 CPU autograd of the same model on the engine path, same roots
    mc, _, _ = _setup("cpu", data_dir)
    mc.load_state_dict(state)
    raw = torch.as_tensor(np.asarray(g.ids)[roots.numpy()].astype(np.int64))
    logits = mc.out_fc(mc.embed(raw)).float()
    y = ge.get_dense_feature(raw, [mc.label_idx], [mc.label_dim])[0].float()
    ref_loss = F.binary_cross_entropy_with_logits(logits, y)
    ref_loss.backward()
    ref = {n: p.grad.detach().clone() for n, p in mc.named_parameters()}
    assert set(ref) == set(grads) and any("sparse_embeddings" in n for n in ref) and \
        any(n.endswith("_node_encoder.embedding.weight") for n in ref)
    assert all(float(r.norm()) > 0 for n, r in ref.items() if "embedding" in n)
    print("loss", float(loss.detach()), float(ref_loss.detach()))
    loss, ref_loss = float(loss.detach()), float(ref_loss.detach())
    assert abs(loss - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    for n, gr in grads.items():
        r = ref[n]
        err = float((gr - r).norm() / max(float(r.norm()), 1e-12))
        print(n, err)
        assert err < 1e-3, (n, err)


@pytest.mark.gpu
def test_sparse_geniepath_replay_matches_eager(data_dir):
    """10. hipGraph capture + replays of the sparse + id GeniePath step against eager steps"""
    from euler_amd.models.encoder_trainer import EncoderFlowTrainer

    losses = []
    for captured in (False, True):
        m, est, g = _setup("cuda", data_dir)
        tr = EncoderFlowTrainer.from_model(m, g, 64, learning_rate=0.01)
        out = []
        if captured:
            tr.capture(warmup=2, steps=4)
            out += [None, None]
            for _ in range(6):
                tr.replay(1)
                out.append(float(tr.loss.item()))
        else:
            for _ in range(8):
                tr.step()
                out.append(float(tr.loss.item()))
        losses.append(out)
    eager, graph = losses
    print("eager", eager, "graph", graph)
    np.testing.assert_allclose(graph[2:], eager[2:], rtol=1e-4, atol=1e-5)


@pytest.mark.gpu
def test_sparse_geniepath_step_matches_cpu_oracle(data_dir):
    """11. one device step's loss and gradients (table gradients included) = fp32 CPU
    autograd of the same model on the engine path for the same roots"""
    _step_vs_cpu_oracle("cuda", data_dir)


def _estimator_case(device, tmp_path, model, kind, caplog):
    """20 steps through the runner, every step logged (the eager warm-up steps before a
    hipGraph capture are not: the first logged value is then the first captured step's).
    DGI's corrupted view is one random permutation shared by the whole batch, so its
    per-step loss is noisy whatever the batch size: a small learning rate keeps 20 steps a
    descent."""
    from euler_amd.tools import runner

    lr = {"geniepath": "0.01", "dgi": "0.001"}[model]
    a = runner.parse_args(["--dataset", "cora_sparse", "--scale", "0.05", "--batch_size", "256", "--log_steps", "1",
                           "--device", device, "--seed", "1", "--model_dir", str(tmp_path / "ckpt"), "--data_dir",
                           str(tmp_path / "data"), "--device_graph", "--total_step", "20", "--learning_rate", lr,
                           "--use_sparse_feature"], model=model)
    _, est = runner.build(a)
    with caplog.at_level(logging.INFO):
        res = est.train()
    logged = [float(x) for x in re.findall(r"step = \d+, loss = ([0-9.eE+-]+|nan|inf)", caplog.text)]
    print(model, logged)
    assert res["step"] == 20 and 2 <= len(logged) <= 20 and all(math.isfinite(x) for x in logged)
    assert abs(logged[-1] - res["loss"]) < 1e-5
    assert est.device_trainer.device_trainer_kind == kind
    assert logged[-1] < logged[0], logged


@pytest.mark.gpu
@pytest.mark.parametrize("model,kind", [("geniepath", "encoder_flow"), ("dgi", "dgi")])
def test_estimator_sparse_inputs_gpu(tmp_path, monkeypatch, caplog, model, kind):
    """12. NodeEstimator(device_graph=True) over --use_sparse_feature on the GPU"""
    monkeypatch.chdir(tmp_path)
    _estimator_case("cuda", tmp_path, model, kind, caplog)
