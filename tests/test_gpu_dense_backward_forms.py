"""The dense tail of the backward in its fused forms against the launches they replace, bit for bit (torch.equal
everywhere):
 - ops.gemm_tn_bn_bwd (BatchNorm's input gradient formed inside the dW GEMM) against bwd_apply + gemm_tn(colsum=True);
 - ops.gemm_tn_rows (the product over a row list) against the full product with the other rows zeroed — equal only if
   v_mfma_f32_32x32x2_f32 adds its two k-steps in order, which this test decides;
 - whole training steps with ops.FUSE_DENSE_BACKWARD on against off, eager and replayed from a captured hipGraph."""
import copy

import pytest
import torch

from rgb_experiment_amd import ops
from rgb_experiment_amd.nn import batchnorm as B

pytestmark = pytest.mark.gpu

# K = 1, 31, 33: one ragged tile / two tiles in ONE slab; 4 000: 8 slabs; 70 001: 137 slabs of 512 rows, the last one
# ragged (481 rows: 15 tiles and one row)
KS = [1, 31, 33, 4000, 70001]
SHAPES = [(128, 128), (64, 128), (32, 64)]  # the 128-row tile, the 64-row tile, the 64-row tile half empty


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _operands(dev, K, M, N, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(K, M, generator=g).to(dev), torch.randn(K, M, generator=g).to(dev),
            torch.randn(K, N, generator=g).to(dev))


def _constants(dev, M, which, seed=3):
    g = torch.Generator().manual_seed(seed)
    mean, rstd, ca, cb, ck = (torch.randn(M, generator=g), torch.rand(M, generator=g) + 0.5,
                              torch.randn(M, generator=g) * 0.1, torch.randn(M, generator=g) * 0.1,
                              torch.randn(M, generator=g))
    if which == "cb0":
        cb = torch.zeros(M)
    if which == "bigmean":  # x - mean cancels nothing: the products' rounding is all that is left
        mean = mean * 1e4 + 3e4
    return tuple(t.to(dev) for t in (mean, rstd, ca, cb, ck))


@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("K", KS)
def test_bn_bwd_gemm_matches_apply_then_gemm(dev, K, M, N):
    g, x, b = _operands(dev, K, M, N, K + M)
    assert ops._gemm_tn_v4(g, x, b)
    for which in ("plain", "cb0", "bigmean"):
        c = _constants(dev, M, which)
        want_w, want_s = ops.gemm_tn(B.bwd_apply(g, x, *c), b, colsum=True)
        got_w, got_s = ops.gemm_tn_bn_bwd(g, x, *c, b, colsum=True)
        assert torch.equal(got_w, want_w), which
        assert torch.equal(got_s, want_s), which
    got_w, none = ops.gemm_tn_bn_bwd(g, x, *c, b)
    assert none is None and torch.equal(got_w, want_w)


def test_bn_bwd_gemm_unaligned_operands_take_the_two_launches(dev, monkeypatch):
    K, M, N = 4000, 128, 128
    g, x, b = _operands(dev, K, M + 4, N, 9)
    c = _constants(dev, M, "plain")
    called = []
    orig = B.bwd_apply
    monkeypatch.setattr(B, "bwd_apply", lambda *a: called.append(1) or orig(*a))
    for gv, xv, cv in ((g[:, 1:M + 1], x[:, :M], c), (g[:, :M], x[:, 2:M + 2], c),          # rows off the 16-byte grid
                       (g[:, :30], x[:, :30], tuple(t[:30].contiguous() for t in c))):        # width % 4 != 0
        assert not ops._gemm_tn_v4(gv, xv, b)
        n0 = len(called)
        got_w, got_s = ops.gemm_tn_bn_bwd(gv, xv, *cv, b, colsum=True)
        assert len(called) == n0 + 1
        want_w, want_s = ops.gemm_tn(orig(gv, xv, *cv), b, colsum=True)
        assert torch.equal(got_w, want_w) and torch.equal(got_s, want_s)
    # strided but aligned rows (a column block of a wider matrix) stay on the fused form
    n0 = len(called)
    got_w, got_s = ops.gemm_tn_bn_bwd(g[:, 4:M + 4], x[:, :M], *c, b, colsum=True)
    assert len(called) == n0
    want_w, want_s = ops.gemm_tn(orig(g[:, 4:M + 4], x[:, :M], *c), b, colsum=True)
    assert torch.equal(got_w, want_w) and torch.equal(got_s, want_s)


def _row_lists(K, seed):
    g = torch.Generator().manual_seed(seed)
    lists = {"empty": torch.zeros(0, dtype=torch.long), "one": torch.tensor([K // 2]), "all": torch.arange(K),
             "p60": (torch.rand(K, generator=g) < 0.6).nonzero().reshape(-1)}
    # slabs are 512 rows at these sizes (at least 16 tiles of 32 rows each): every other row of the second slab, or of
    # the only one
    lo, hi = (512, 1024) if K > 1024 else (0, K)
    lists["one_slab"] = torch.arange(lo, hi, 2)
    tail = (torch.rand(K, generator=g) < 0.3).nonzero().reshape(-1)
    lists["ends_at_last_row"] = torch.unique(torch.cat([tail, torch.tensor([K - 1])]))
    return lists


@pytest.mark.parametrize("M,N", SHAPES)
@pytest.mark.parametrize("K", KS)
def test_row_list_gemm_matches_full_gemm_on_zeroed_rows(dev, K, M, N):
    a, _, b = _operands(dev, K, M, N, K + N)
    for name, rows in _row_lists(K, K).items():
        sel = torch.zeros(K, dtype=torch.bool)
        sel[rows] = True
        az = torch.where(sel.to(dev)[:, None], a, torch.zeros_like(a))  # the deselected rows zeroed
        want_w, want_s = ops.gemm_tn(az, b, colsum=True)
        got_w, got_s = ops.gemm_tn_rows(az, b, rows.to(dev).to(torch.int32), colsum=True)
        assert torch.equal(got_w, want_w), name
        assert torch.equal(got_s, want_s), name
    assert torch.equal(ops.gemm_tn_rows(az, b, None), want_w)  # no list: the full product


# ---- whole training steps ----------------------------------------------------------------------------------------

N_NODES, N_EDGES, D = 20_000, 400_000, 128


@pytest.fixture(scope="module")
def data(dev):
    g = torch.Generator().manual_seed(11)
    ei = torch.randint(0, N_NODES, (2, N_EDGES), generator=g).to(dev)
    x = torch.randn(N_NODES, D, generator=g).to(dev)
    y = torch.randint(0, D, (N_NODES,), generator=g).to(dev)
    mask = (torch.rand(N_NODES, generator=g) < 0.6).to(dev)
    return ei, x, y, mask


def _model(dev, name, layers):
    from rgb_experiment_amd.models import REGISTRY
    torch.manual_seed(14530529)
    return REGISTRY[name](num_layers=layers, hidden_unit=D, dropout_rate=0.5, input_dim=D, output_dim=D).to(dev)


def _train_step(model, x, ei, y, mask):
    from rgb_experiment_amd.models._stack import masked_ce
    model.train()
    model.zero_grad(set_to_none=True)
    if x.requires_grad:
        x.grad = None
    loss, stats = masked_ce(model, {"x": x, "edge_index": ei}, y, mask)
    loss.backward()
    out = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    out.update({k: v.clone() for k, v in model.named_buffers()})  # BatchNorm's running statistics
    if x.requires_grad:
        out["x.grad"] = x.grad.clone()
    return loss.detach().clone(), stats.clone(), out


def _count_calls(monkeypatch):
    calls = {"fused": 0, "rows": 0, "apply": 0}
    fused, rows, apply = ops.gemm_tn_bn_bwd, ops.gemm_tn_rows, B.bwd_apply

    def count(key, fn, hit=lambda a, k: True):
        def wrapper(*a, **k):
            calls[key] += bool(hit(a, k))
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(ops, "gemm_tn_bn_bwd", count("fused", fused))
    monkeypatch.setattr(ops, "gemm_tn_rows", count("rows", rows, lambda a, k: a[2] is not None))
    monkeypatch.setattr(B, "bwd_apply", count("apply", apply))
    return calls


@pytest.mark.parametrize("name,layers,x_grad", [("gcn", 2, False), ("graphsage", 2, False), ("gcn", 3, False),
                                                ("gcn", 2, True)])
def test_training_step_switch_on_equals_off(dev, data, monkeypatch, name, layers, x_grad):
    ei, x, y, mask = data
    x = x.clone().requires_grad_() if x_grad else x
    model = _model(dev, name, layers)
    twin = copy.deepcopy(model)
    calls = _count_calls(monkeypatch)
    assert ops.FUSE_DENSE_BACKWARD
    loss1, stats1, out1 = _train_step(model, x, ei, y, mask)
    on = dict(calls)
    monkeypatch.setattr(ops, "FUSE_DENSE_BACKWARD", False)
    loss0, stats0, out0 = _train_step(twin, x, ei, y, mask)
    off = {k: calls[k] - on[k] for k in calls}
    assert torch.equal(loss1, loss0)
    assert torch.equal(stats1, stats0)
    assert out1.keys() == out0.keys() and any(k.endswith("bns.0.weight") for k in out1)
    for k in out0:
        assert torch.equal(out1[k], out0[k]), k
    # the forms really ran / really stayed away: the first GCN layer of a model whose input takes no gradient folds the
    # apply pass into dW; a root weight (SAGE) or an input gradient keeps the apply kernel; dW of the last layer runs
    # over the row list either way
    assert off == {"fused": 0, "rows": 0, "apply": layers - 1}
    assert on["rows"] == 1
    if name == "gcn" and not x_grad:
        assert on["fused"] == 1 and on["apply"] == layers - 2
    else:
        assert on["fused"] == 0 and on["apply"] == layers - 1


def test_graphed_epoch_switch_on_equals_off(dev, data, monkeypatch):
    from rgb_experiment_amd.epoch_graph import GraphedEpoch
    ei, x, y, mask = data
    masks = (mask, ~mask, ~mask)
    results = []
    for switch in (True, False):
        monkeypatch.setattr(ops, "FUSE_DENSE_BACKWARD", switch)
        model = _model(dev, "gcn", 2)
        if switch:
            loss_eager = _train_step(copy.deepcopy(model), x, ei, y, mask)[0]
        opt = torch.optim.Adam(model.parameters(), lr=0.01, capturable=True)
        calls = _count_calls(monkeypatch)
        ge = GraphedEpoch(model, opt, {"x": x, "edge_index": ei}, y, masks).capture(warmup=1)
        if switch:  # warm-up + capture: the fused forms are what was captured
            assert calls["fused"] == 2 and calls["rows"] == 2 and calls["apply"] == 0
        first = ge.run()
        second = ge.run()
        torch.cuda.synchronize()
        results.append((first, second, {k: v.detach().clone() for k, v in model.state_dict().items()}))
        monkeypatch.undo()
    (f1, s1, sd1), (f0, s0, sd0) = results
    assert f1 == f0 and s1 == s0
    # the first replay starts from the eager step's parameters: the same training loss (nll sum / rows, rounded to fp32)
    assert torch.tensor(f1[0], dtype=torch.float64).float().item() == loss_eager.item()
    for k in sd0:
        assert torch.equal(sd1[k], sd0[k]), k
