"""The last layer's fused kernel gathering only the rows its masked cross-entropy selects (rgbx_ce_epilogue_t.rows /
skip_unselected) and the backward's transposed gather skipping the columns it does not select (rgbx_fused_layer_t.col_sel),
against the full forms they replace.

Exactness: statistics counts and hits exact, the nll sum to fp64 rounding (its tile records are added in another order);
the loss gradient, the stored aggregate of selected rows and dW bit-identical; the transposed gather with the column
selection bit-identical to the full one (every slot keeps its place in the sum); whole training steps: loss, statistics
and every gradient bit-identical."""
import copy

import pytest
import torch

from rgb_experiment_amd import ops
from rgb_experiment_amd.graph import LONG_ROW_SLOTS, Graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _graph(dev, n=4000, e=60000, seed=0, hub=True, loops_mode=1):
    """Random edges whose targets avoid the last tenth of the nodes (isolated targets); one hub target above the
    row-split threshold in the forward CSR and one hub source in the transposed one."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n - n // 10, (e,), generator=g)
    if hub:
        k = 3 * LONG_ROW_SLOTS
        src = torch.cat([src, torch.randint(0, n, (k,), generator=g), torch.full((k,), 11)])
        dst = torch.cat([dst, torch.full((k,), 5), torch.randint(0, n - n // 10, (k,), generator=g)])
    ei = torch.stack([src, dst]).to(dev)
    return Graph(ei, n, loops_mode)


def _labels(dev, n, C, seed=1):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (n,), generator=g)
    y[::17] = C       # out of range: deselects the row
    y[7::23] = -1
    return y.to(dev)


def _masks(dev, n, seed=2):
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(n, generator=g)
    one = torch.zeros(n, dtype=torch.bool)
    one[5] = True  # the hub row alone
    return {"empty": torch.zeros(n, dtype=torch.bool).to(dev), "one": one.to(dev), "p20": (r < 0.2).to(dev),
            "all": torch.ones(n, dtype=torch.bool).to(dev)}


def _stats_pair(x, wt, graph, w, y, mask, bias, root):
    kw = dict(csr=graph.fwd, w=w, bias=bias, x_root=x if root else None, wt_root=wt if root else None,
              ce=(y, mask, None))
    _, _, full = ops.fused_layer(x, wt, **kw)
    _, _, rows = ops.fused_layer(x, wt, select_rows=True, **kw)
    return full, rows


def _check_stats(full, rows):
    full, rows = full.reshape(-1, 3).cpu(), rows.reshape(-1, 3).cpu()
    assert torch.equal(full[:, 1:], rows[:, 1:])  # counts and hits exact
    torch.testing.assert_close(rows[:, 0], full[:, 0], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("K", [32, 64, 128, 256])
@pytest.mark.parametrize("n_out", [32, 128])
def test_row_list_statistics_match_full_tiles(dev, K, n_out):
    graph = _graph(dev)
    n = graph.N
    g = torch.Generator().manual_seed(K + n_out)
    x = torch.randn(n, K, generator=g).to(dev)
    wt = (torch.randn(K, n_out, generator=g) / K ** 0.5).to(dev)
    bias = torch.randn(n_out, generator=g).to(dev)
    y = _labels(dev, n, n_out)
    masks = _masks(dev, n)
    for name, mask in masks.items():
        full, rows = _stats_pair(x, wt, graph, graph.w, y, mask, bias, False)
        _check_stats(full, rows)
        if name == "empty":
            assert rows.reshape(-1)[1].item() == 0
    # two statistics sets from one forward: the list is the union of both masks
    full, rows = _stats_pair(x, wt, graph, graph.w, y, (masks["p20"], ~masks["p20"] & masks["all"]), bias, False)
    _check_stats(full, rows)


def test_row_list_statistics_with_root_term(dev):
    graph = _graph(dev, loops_mode=0)
    n, K, C = graph.N, 128, 128
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, K, generator=g).to(dev)
    wt = (torch.randn(K, C, generator=g) / K ** 0.5).to(dev)
    y = _labels(dev, n, C)
    for mask in _masks(dev, n).values():
        full, rows = _stats_pair(x, wt, graph, None, y, mask, None, True)
        _check_stats(full, rows)


@pytest.mark.parametrize("with_pre", [False, True])
def test_gradient_form_skips_unselected_rows(dev, with_pre):
    graph = _graph(dev)
    n, K, C = graph.N, 128, 128
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, K, generator=g).to(dev)
    wt = (torch.randn(K, C, generator=g) / K ** 0.5).to(dev)
    bias = torch.randn(C, generator=g).to(dev)
    y = _labels(dev, n, C)
    mask = _masks(dev, n)["p20"]
    pre = None
    if with_pre:
        pre = (torch.rand(K, generator=g).to(dev) + 0.5, torch.randn(K, generator=g).to(dev), graph.rowsum("gcn"))
    scale = ops.mask_scale(y, mask, C)
    kw = dict(csr=graph.fwd, w=graph.w, bias=bias, pre=pre, want_z=True, ce=(y, mask, scale))
    d0, z0, s0 = ops.fused_layer(x, wt, **kw)
    d1, z1, s1 = ops.fused_layer(x, wt, select_rows=True, **kw)
    sel = ops.ce_selection(y, mask, C)
    assert torch.equal(d0, d1)
    assert torch.equal(s0, s1)
    assert torch.equal(z1[sel], z0[sel])
    assert torch.count_nonzero(z1[~sel]).item() == 0
    assert torch.equal(ops.gemm_tn(d0, z0), ops.gemm_tn(d1, z1))


@pytest.mark.parametrize("kind", ["gcn", "mean"])
def test_column_selection_matches_full_transposed_gather(dev, kind):
    graph = _graph(dev, loops_mode=1 if kind == "gcn" else 0)
    n, C = graph.N, 128
    y = _labels(dev, n, C)
    mask = (torch.rand(n, generator=torch.Generator().manual_seed(4)) < 0.6).to(dev)
    sel = ops.selected_cols(y, mask, C)
    assert torch.equal(sel.bool(), ops.ce_selection(y, mask, C))
    w = graph.w_t if kind == "gcn" else graph.w_mean_t
    g = torch.Generator().manual_seed(5)
    gy = (torch.randn(n, C, generator=g).to(dev) * sel[:, None]).contiguous()  # the loss gradient: 0 where deselected
    wt = (torch.randn(C, C, generator=g) / C ** 0.5).to(dev)
    full, _, _ = ops.fused_layer(gy, wt, csr=graph.bwd, w=w)
    cut, _, _ = ops.fused_layer(gy, wt, csr=graph.bwd, w=w, col_sel=sel)
    assert torch.equal(cut, full)
    if kind == "mean":  # SAGE: the root term reads dy itself
        full, _, _ = ops.fused_layer(gy, wt, csr=graph.bwd, w=w, x_root=gy, wt_root=wt)
        cut, _, _ = ops.fused_layer(gy, wt, csr=graph.bwd, w=w, x_root=gy, wt_root=wt, col_sel=sel)
        assert torch.equal(cut, full)


def test_mask_edit_rebuilds_list_and_selection(dev):
    n, C = 2000, 32
    y = _labels(dev, n, C)
    mask = _masks(dev, n)["p20"].clone()
    rows0 = ops.selected_rows(y, mask, C).clone()
    sel0 = ops.selected_cols(y, mask, C).clone()
    mask[: n // 2] = False  # in place: the version moves
    rows1 = ops.selected_rows(y, mask, C)
    sel1 = ops.selected_cols(y, mask, C)
    want = ops.ce_selection(y, mask, C)
    assert torch.equal(rows1.long(), want.nonzero().reshape(-1))
    assert torch.equal(sel1.bool(), want)
    assert rows1.numel() < rows0.numel()
    assert int(sel1.sum()) < int(sel0.sum())


def _train_step(model, x, ei, y, mask, seed):
    from rgb_experiment_amd.models._stack import masked_ce
    torch.manual_seed(seed)
    model.train()
    model.zero_grad(set_to_none=True)
    loss, stats = masked_ce(model, {"x": x, "edge_index": ei}, y, mask)
    loss.backward()
    return loss.detach().clone(), stats.clone(), {k: p.grad.clone() for k, p in model.named_parameters()
                                                 if p.grad is not None}


@pytest.mark.parametrize("name", ["gcn", "graphsage"])
def test_training_step_matches_full_gather(dev, name, monkeypatch):
    from rgb_experiment_amd.models import REGISTRY
    n, e, d = 200_000, 4_000_000, 128  # workload S
    g = torch.Generator().manual_seed(11)
    ei = torch.randint(0, n, (2, e), generator=g).to(dev)
    x = torch.randn(n, d, generator=g).to(dev)
    y = torch.randint(0, d, (n,), generator=g).to(dev)
    mask = (torch.rand(n, generator=g) < 0.6).to(dev)
    torch.manual_seed(14530529)
    model = REGISTRY[name](num_layers=2, hidden_unit=128, dropout_rate=0.5, input_dim=d, output_dim=d).to(dev)
    twin = copy.deepcopy(model)
    loss1, stats1, grads1 = _train_step(model, x, ei, y, mask, 5)
    # the full path: every row and every transposed slot gathered
    orig = ops.fused_layer
    monkeypatch.setattr(ops, "fused_layer", lambda *a, **k: orig(*a, **{**k, "select_rows": False, "col_sel": None}))
    loss0, stats0, grads0 = _train_step(twin, x, ei, y, mask, 5)
    assert torch.equal(loss1, loss0)
    assert torch.equal(stats1, stats0)
    assert grads1.keys() == grads0.keys()
    for k in grads0:
        assert torch.equal(grads1[k], grads0[k]), k
