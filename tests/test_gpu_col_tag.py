"""The column selection carried in the transposed column stream (rgbx_col_tag_i32, rgbx_fused_layer_t.col_tag) and the
row-list loss gradient without its zero fill (rgbx_ce_epilogue_t.no_fill), against the forms they replace.

Every comparison is torch.equal: a tagged slot keeps its place in the sum exactly as a looked-up one does, and a row that
is not written is a row nobody reads. Host side: tests/test_transposed_col_tag_host.py."""
import copy

import pytest
import torch

from rgb_experiment_amd import _lib, ops
from rgb_experiment_amd.graph import CSR, Graph, make_row_split

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


N_NODES = 3001       # no multiple of the 32-row tile
FORCED = list(range(100, 140)) + [200, 201]  # columns every non-empty mask selects (never multiples of 17)
ROW_CANCEL = 8       # slots = columns 200, 201, whose dy rows are v and -v


def _labels(C, n=N_NODES):
    y = torch.randint(0, C, (n,), generator=torch.Generator().manual_seed(1))
    y[::17] = C      # outside [0, C): deselected under every mask
    y[7::23] = -1
    y[FORCED] = 3
    return y


def _masks(n=N_NODES):
    r = torch.rand(n, generator=torch.Generator().manual_seed(2)) < 0.6
    r[FORCED] = True
    return {"0": torch.zeros(n, dtype=torch.bool), "60": r, "100": torch.ones(n, dtype=torch.bool)}


def _hand_csr(dev, threshold=None):
    """Square CSR over N_NODES rows, about 40 000 slots: hand-placed rows first, random ones behind them."""
    g = torch.Generator().manual_seed(3)
    n = N_NODES
    dead = torch.tensor([c for c in range(0, n, 17) if c not in FORCED])  # always deselected (label out of range)
    pick = lambda k: torch.randint(0, n, (k,), generator=g)
    rows = [pick(0), pick(1), pick(63), pick(64), pick(65), pick(200),          # rows 0..5: batch boundaries, 4 batches
            dead[torch.randint(0, dead.numel(), (37,), generator=g)],           # row 6: every slot deselected
            torch.tensor([100 + i if i % 4 == 0 else int(dead[i]) for i in range(40)]),  # row 7: the selected slots share
            torch.tensor([200, 201])]                                           # one residue mod NG; row 8: v and -v
    deg = torch.randint(0, 27, (n - len(rows),), generator=g)
    rows += [pick(int(k)) for k in deg]
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([r.numel() for r in rows]), 0)
    col = torch.cat(rows).to(torch.int32)
    nnz = col.numel()
    rowptr = rowptr.to(torch.int32).to(dev)
    split = None if threshold is None else make_row_split(rowptr, threshold)
    return CSR(rowptr, col.to(dev), torch.arange(nnz, dtype=torch.int32, device=dev), n, nnz, split)


def _weights(kind, csr, dev):
    """Per-slot weights >= 0 as the three kinds of the transposed launch have them; equal on the two slots of ROW_CANCEL."""
    if kind == "sum":
        return None
    g = torch.Generator().manual_seed(4)
    if kind == "gcn":
        dis = torch.rand(csr.N, generator=g) + 0.1
        rowid = torch.repeat_interleave(torch.arange(csr.N), (csr.rowptr[1:] - csr.rowptr[:-1]).cpu().long())
        w = dis[rowid] * dis[csr.col.cpu().long()]
    else:  # mean: 1 / degree of the slot's column
        cnt = torch.bincount(csr.col.cpu().long(), minlength=csr.N).clamp(min=1)
        w = 1.0 / cnt[csr.col.cpu().long()].float()
    p = int(csr.rowptr[ROW_CANCEL].item())
    w[p + 1] = w[p]
    return w.float().to(dev)


def _dy(sel, K, dev):
    """A loss gradient: zero (some of it -0.0) outside the selected rows, with -0.0 entries inside and one exactly
    cancelling pair of rows."""
    g = torch.Generator().manual_seed(5)
    gy = torch.randn(N_NODES, K, generator=g)
    gy[torch.rand(N_NODES, K, generator=g) < 0.05] = -0.0
    gy[201] = -gy[200]
    gy = gy * sel.cpu()[:, None].float()
    gy[::34] = -0.0  # deselected rows (multiples of 17) holding negative zeros
    return gy.to(dev).contiguous()


def _want_tag(col, sel):
    c = col.long()
    return torch.where(sel[c].bool(), c, ~c).to(torch.int32)


def _tag(col, sel, n_cols=None):
    out = torch.full((max(col.numel(), 1),), 12345, dtype=torch.int32, device=sel.device)
    _lib.check(_lib.load().rgbx_col_tag_i32(col.data_ptr(), sel.data_ptr(), col.numel(), sel.numel() if n_cols is None
                                            else n_cols, out.data_ptr(), _lib.stream_ptr()), "rgbx_col_tag_i32")
    return out[:col.numel()]


def test_tag_kernel(dev):
    csr = _hand_csr(dev)
    g = torch.Generator().manual_seed(6)
    for sel in ((torch.rand(N_NODES, generator=g) < 0.6), torch.ones(N_NODES, dtype=torch.bool),
                torch.zeros(N_NODES, dtype=torch.bool)):
        sel = sel.to(torch.uint8).to(dev)
        got = _tag(csr.col, sel)
        assert torch.equal(got, _want_tag(csr.col, sel))
        assert torch.equal(torch.where(got < 0, ~got, got), csr.col)  # the column stays recoverable
    assert torch.equal((_tag(csr.col, torch.ones(N_NODES, dtype=torch.uint8, device=dev)) >= 0).cpu(),
                       torch.ones(csr.nnz, dtype=torch.bool))
    assert _tag(csr.col[:0], sel).numel() == 0  # nnz = 0: no launch, no error
    # a column past the selection vector counts as deselected and never comes out non-negative
    short = _tag(csr.col, torch.ones(1000, dtype=torch.uint8, device=dev))
    assert torch.equal(short >= 0, csr.col < 1000)


def _three_ways(gy, wt, csr, w, y, mask, C):
    """The transposed launch without selection, with col_sel looked up per slot, and with the tagged column stream."""
    sel = ops.selected_cols(y, mask, C)
    full, _, _ = ops.fused_layer(gy, wt, csr=csr, w=w)
    looked, _, _ = ops.fused_layer(gy, wt, csr=csr, w=w, col_sel=sel.clone())  # not selected_cols' own vector: no tag
    key = (csr.col.data_ptr(), csr.nnz, ops._sel_key(y, mask, C))
    assert key not in ops._COL_TAGS or ops._COL_TAGS[key][2] is sel
    tagged, _, _ = ops.fused_layer(gy, wt, csr=csr, w=w, col_sel=sel)
    assert key in ops._COL_TAGS, "the tagged launch did not run"
    assert torch.equal(ops._COL_TAGS[key][0].value, _want_tag(csr.col, sel))
    return full, looked, tagged


@pytest.mark.parametrize("kind", ["gcn", "mean", "sum"])
@pytest.mark.parametrize("K, n_out", [(64, 64), (128, 128), (256, 128)])
@pytest.mark.parametrize("hubs", [False, True])
def test_tagged_transposed_launch_matches(dev, K, n_out, kind, hubs):
    """`hubs`: a split plan whose threshold (60) makes the rows of 63, 64, 65 and 200 slots hub rows: they read `col`,
    never a tagged entry."""
    csr = _hand_csr(dev, threshold=60 if hubs else None)
    assert (csr.split is not None and csr.split["n_long"] >= 4) if hubs else csr.split is None
    w = _weights(kind, csr, dev)
    wt = (torch.randn(K, n_out, generator=torch.Generator().manual_seed(K)) / K ** 0.5).to(dev)
    y = _labels(K).to(dev)
    for name, mask in _masks().items():
        mask = mask.to(dev)
        sel = ops.ce_selection(y, mask, K)
        assert (int(sel.sum()) == 0) == (name == "0")
        gy = _dy(sel, K, dev)
        full, looked, tagged = _three_ways(gy, wt, csr, w, y, mask, K)
        assert torch.equal(looked, full), name
        assert torch.equal(tagged, full), name
        assert torch.count_nonzero(full[0]).item() == 0 and torch.count_nonzero(full[6]).item() == 0
        if kind == "sum" or K < 256:
            # v and -v under equal weights cancel to +0: added as they are ('sum'), or as two separately rounded products
            # in two lane groups (NG >= 2). With one group (K = 256) the second fmaf sees the first's rounding error.
            assert torch.count_nonzero(full[ROW_CANCEL]).item() == 0


def _random_graph(dev, n, e, seed):
    ei = torch.randint(0, n, (2, e), generator=torch.Generator().manual_seed(seed)).to(dev)
    return Graph(ei, n, 1), ei


def test_no_fill_leaves_unlisted_rows_alone(dev):
    graph, _ = _random_graph(dev, 4001, 40000, 7)
    n, K, C = graph.N, 128, 128
    assert graph.bwd.split is None
    g = torch.Generator().manual_seed(8)
    x = torch.randn(n, K, generator=g).to(dev)
    wt = (torch.randn(K, C, generator=g) / K ** 0.5).to(dev)
    bias = torch.randn(C, generator=g).to(dev)
    y = _labels(C, n).to(dev)
    mask = (torch.rand(n, generator=g) < 0.6).to(dev)
    scale = ops.mask_scale(y, mask, C)
    sel = ops.ce_selection(y, mask, C)
    rows = ops.selected_rows(y, mask, C)
    kw = dict(csr=graph.fwd, w=graph.w, bias=bias, ce=(y, mask, scale), select_rows=True)
    d0, z0, s0 = ops.fused_layer(x, wt, want_z=True, **kw)
    assert torch.count_nonzero(d0[~sel]).item() == 0 and torch.count_nonzero(z0[~sel]).item() == 0  # the default fills
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    d1, z1, s1 = ops.fused_layer(x, wt, out=nan(n, C), z=nan(n, K), ce_fill=False, **kw)
    assert torch.equal(s1, s0)
    assert torch.equal(d1[sel], d0[sel]) and torch.equal(z1[sel], z0[sel])
    assert bool(torch.isnan(d1[~sel]).all()) and bool(torch.isnan(z1[~sel]).all())  # nothing was written there
    gw0, gb0 = ops.gemm_tn_rows(d0, z0, rows, colsum=True)
    gw1, gb1 = ops.gemm_tn_rows(d1, z1, rows, colsum=True, rows_only=True)
    assert torch.equal(gw1, gw0) and torch.equal(gb1, gb0)
    cols = ops.selected_cols(y, mask, C)
    h0, _, _ = ops.fused_layer(d0, wt, csr=graph.bwd, w=graph.w_t, col_sel=cols)
    h1, _, _ = ops.fused_layer(d1, wt, csr=graph.bwd, w=graph.w_t, col_sel=cols)
    assert (graph.bwd.col.data_ptr(), graph.bwd.nnz, ops._sel_key(y, mask, C)) in ops._COL_TAGS
    assert torch.equal(h1, h0) and not bool(torch.isnan(h1).any())
    hl, _, _ = ops.fused_layer(d1, wt, csr=graph.bwd, w=graph.w_t, col_sel=cols.clone())  # looked up per slot: as safe
    assert torch.equal(hl, h0)


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
def test_training_step_without_fill(dev, name, monkeypatch):
    """gcn: the last layer's forward asks for no fill (its buffers are poisoned with NaN here), and the step equals the one
    with CE_GRAD_ROW_LIST off in loss, statistics and every gradient. graphsage (root weight: dWr and the root term read
    every row of dy) keeps filling."""
    from rgb_experiment_amd.models import REGISTRY
    n, e, d = 20_000, 400_000, 128
    g = torch.Generator().manual_seed(11)
    ei = torch.randint(0, n, (2, e), generator=g).to(dev)
    x = torch.randn(n, d, generator=g).to(dev)
    y = torch.randint(0, d, (n,), generator=g).to(dev)
    mask = (torch.rand(n, generator=g) < 0.6).to(dev)
    torch.manual_seed(14530529)
    model = REGISTRY[name](num_layers=2, hidden_unit=128, dropout_rate=0.5, input_dim=d, output_dim=d).to(dev)
    twin = copy.deepcopy(model)
    orig = ops.fused_layer
    asked = []

    def spy(x_, wt_, **k):
        if k.get("ce") is not None and k["ce"][2] is not None:  # the loss-gradient launch
            asked.append(not k.get("ce_fill", True))
            if asked[-1]:
                assert k.get("out") is None and k.get("z") is None
                k["out"] = torch.full((k["csr"].N, wt_.size(1)), float("nan"), device=dev)
                k["z"] = torch.full((k["csr"].N, wt_.size(0)), float("nan"), device=dev)
        return orig(x_, wt_, **k)

    monkeypatch.setattr(ops, "fused_layer", spy)
    loss1, stats1, grads1 = _train_step(model, x, ei, y, mask, 5)
    assert asked == [name == "gcn"]
    monkeypatch.setattr(ops, "CE_GRAD_ROW_LIST", False)
    loss0, stats0, grads0 = _train_step(twin, x, ei, y, mask, 5)
    assert asked == [name == "gcn", False]
    assert torch.equal(loss1, loss0)
    assert torch.equal(stats1, stats0)
    assert grads1.keys() == grads0.keys()
    for k in grads0:
        assert not bool(torch.isnan(grads1[k]).any()), k
        assert torch.equal(grads1[k], grads0[k]), k


def test_tag_cache_follows_mask_and_graph(dev):
    C = 64
    a, b = _hand_csr(dev), _hand_csr(dev)  # equal contents, two graphs
    y = _labels(C).to(dev)
    mask = _masks()["60"].to(dev).clone()
    sel0 = ops.selected_cols(y, mask, C)
    t_a = ops.col_tags(a, sel0)
    t_b = ops.col_tags(b, sel0)
    assert t_a is ops.col_tags(a, sel0)  # served again
    assert t_a.data_ptr() != t_b.data_ptr()
    assert torch.equal(t_a, _want_tag(a.col, sel0)) and torch.equal(t_b, _want_tag(b.col, sel0))
    assert len(ops._COL_TAGS) <= 2
    keep = t_a.clone()
    mask[: N_NODES // 2] = False  # in place: the version moves, selected_cols hands out a new vector
    sel1 = ops.selected_cols(y, mask, C)
    assert sel1 is not sel0
    t_a1 = ops.col_tags(a, sel1)
    assert t_a1 is not t_a and torch.equal(t_a1, _want_tag(a.col, sel1)) and not torch.equal(t_a1, keep)
    assert len(ops._COL_TAGS) <= 2
    assert ops.col_tags(a, sel1.clone()) is None  # not selected_cols' vector: looked up per slot


def test_capture_without_a_tag_runs_untagged(dev):
    K = 128
    csr = _hand_csr(dev)
    w = _weights("gcn", csr, dev)
    wt = (torch.randn(K, K, generator=torch.Generator().manual_seed(9)) / K ** 0.5).to(dev)
    y = _labels(K).to(dev)
    mask = _masks()["60"].to(dev).clone()
    sel = ops.selected_cols(y, mask, K)
    gy = _dy(ops.ce_selection(y, mask, K), K, dev)
    eager, _, _ = ops.fused_layer(gy, wt, csr=csr, w=w, col_sel=sel.clone())
    torch.cuda.synchronize()
    key = (csr.col.data_ptr(), csr.nnz, ops._sel_key(y, mask, K))
    assert key not in ops._COL_TAGS
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert ops.col_tags(csr, sel) is None  # not built inside a capture
        out, _, _ = ops.fused_layer(gy, wt, csr=csr, w=w, col_sel=sel)
    assert key not in ops._COL_TAGS
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    tagged, _, _ = ops.fused_layer(gy, wt, csr=csr, w=w, col_sel=sel)  # outside the capture the array is built
    assert key in ops._COL_TAGS and torch.equal(tagged, eager)
