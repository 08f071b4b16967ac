"""GINEConv on the MI355X: ops.gine_aggregate (every vector width and group count of the lane layout, hub rows in both
CSRs, rows of exactly 0 / 1 / 64 / 65 / T / T + 1 slots, rows without in-edges, sources without out-edges, graphs of one
to three nodes, a graph without edges, planted ties, width 300 through the column blocks), g_e bit for bit, selective
backward passes, strided and offset operands, ops.edge_rows_to_slots, GINEConv, the GINE model and
experiment(model_name="gine", use_edge_attr=True) against the float64 restatement of tests/test_gine_host.py. The cases
are that file's; it checks on the CPU that each is well-posed.

Tolerances are the project's for this depth of fp32 gather (tests/test_gpu_transformer.py): forward
1e-4 * max(1, |ref|max), gradients 2e-4 * max(1, |ref|max). Every element is compared.

Rows the kernels have no slot for. The op allocates its output and its gradients with torch.empty. Before every operator
call the allocator's free blocks of those sizes ([N, C] and [E, C]) are filled with NaN (`poison`), so a row or a slot
that a kernel skipped shows as NaN in the comparison instead of passing on stale zeros; `finite` is asserted on top."""
import functools

import numpy as np
import pytest
import torch

import test_gine_host as G
import test_transformer_host as T
from test_gpu_ggnn import close, rand_graph
from test_gpu_transformer import device_graph, finite, poison
from test_gine_host import GINE, GINEConv

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = T.FWD_TOL, T.GRAD_TOL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def operator_graph(name, dev):
    """The device graph of a host-file graph, with what the cases rely on asserted once."""
    ei, n = G.graph_of(name)
    graph = device_graph(ei, n, dev)
    assert graph.fwd.nnz == ei.size(1) and graph.bwd.nnz == ei.size(1)        # nothing added, nothing coalesced
    if ei.size(1):   # slot p of the device's CSR is edge order[p] of the host file, in both directions of the map
        assert torch.equal(graph.fwd.perm[:graph.fwd.nnz].cpu().long(), G.slots_of(name)[3])
    if name == "random":
        indeg = (graph.fwd.rowptr[1:] - graph.fwd.rowptr[:-1]).cpu()
        outdeg = (graph.bwd.rowptr[1:] - graph.bwd.rowptr[:-1]).cpu()
        assert bool((indeg[:20] == 0).all()) and bool((outdeg[20:40] == 0).all())
    if name == "powerlaw":
        assert graph.fwd.split is not None and graph.bwd.split is not None    # both chunk paths run
    if name == "degrees":   # exactly one row beyond the threshold in each CSR: T stays whole, T + 1 is split
        indeg = (graph.fwd.rowptr[1:] - graph.fwd.rowptr[:-1]).cpu()
        outdeg = (graph.bwd.rowptr[1:] - graph.bwd.rowptr[:-1]).cpu()
        assert tuple(indeg[:6].tolist()) == G.DEGREES and tuple(outdeg[6:12].tolist()) == G.DEGREES
        assert graph.fwd.split["n_long"] == 1 and graph.bwd.split["n_long"] == 1
    if name == "no_edges":
        assert graph.fwd.nnz == 0
    return graph


def device_case(C, graph_name, dev):
    """(x, e_slot, cot, eps) of a host-file case on the device: e in forward CSR slot order."""
    x, e, cot = G.operator_case(C, graph_name)
    order = G.slots_of(graph_name)[3]
    return (x.float().to(dev), e[order].float().to(dev), cot.float().to(dev),
            torch.tensor([G.EPS], dtype=torch.float32, device=dev))


def run_operator(C, graph_name, dev, needs=(True, True, True), sink=None):
    """ops.gine_aggregate forward and the gradients asked for (`needs`: of x, e_slot, eps); -> (out, [g_x, g_e, g_eps]),
    g_e in forward CSR slot order."""
    from rgb_experiment_amd import ops
    ei, n = G.graph_of(graph_name)
    graph = operator_graph(graph_name, dev)
    x, e, cot, eps = device_case(C, graph_name, dev)
    x, e, eps = (t.requires_grad_(need) for t, need in zip((x, e, eps), needs))
    poison(dev, (n, C), (max(ei.size(1), 1), C))
    if sink is not None:
        ops.set_event_sink(sink)
    try:
        out = ops.gine_aggregate(x, e, graph, eps)
        (out * cot).sum().backward()
    finally:
        ops.set_event_sink(None)
    return out.detach(), [x.grad, e.grad, eps.grad]


def check_operator(C, graph_name, dev):
    out, grads = run_operator(C, graph_name, dev)
    assert finite(out, *grads), "a row or a slot was left unwritten"
    want = G.reference(C, graph_name)
    x, e, cot = G.operator_case(C, graph_name)
    ei, n = G.graph_of(graph_name)
    order = G.slots_of(graph_name)[3]
    assert close(out, want[0], FWD_TOL), "forward"
    assert close(grads[0], want[1][0], GRAD_TOL), "g_x"
    assert grads[1].shape == (ei.size(1), C)
    assert close(grads[2], want[1][2], GRAD_TOL), "g_eps"
    if ei.size(1):
        assert close(grads[1], want[1][1][order], GRAD_TOL), "g_e"
        # no arithmetic happens there: bit for bit the cotangent row of the slot's target, or an exact zero
        mask = (x[ei[0]] + e > 0)[order].to(dev)
        assert torch.equal(grads[1], cot.float().to(dev)[ei[1][order].to(dev)] * mask), "g_e bits"
        k, c = G.tie_positions(ei.size(1), C)                                # planted ties: relu'(0) = 0
        inv = torch.empty_like(order)
        inv[order] = torch.arange(order.numel())
        assert grads[1][inv[k].to(dev), c.to(dev)].abs().max().item() == 0.0
    a = torch.tensor(1 + G.EPS, dtype=torch.float32)
    if graph_name == "no_edges":  # exact: the root term alone
        assert torch.equal(out.cpu(), a * x.float()) and torch.equal(grads[0].cpu(), a * cot.float())
    if graph_name == "random":    # rows without in-edges / sources without out-edges: the root term alone
        assert torch.equal(out[:20].cpu(), a * x.float()[:20])
        assert torch.equal(grads[0][20:40].cpu(), a * cot.float()[20:40])
    return out, grads


@pytest.mark.parametrize("graph", G.GRAPH_NAMES)
@pytest.mark.parametrize("C", G.WIDTHS)
def test_aggregate_forward_backward(dev, C, graph):
    from rgb_experiment_amd import ops
    assert ops.gine_supported(C)
    check_operator(C, graph, dev)


@pytest.mark.parametrize("C", G.DEGREE_WIDTHS)
def test_rows_of_exact_lengths(dev, C):
    """In-degrees and out-degrees of exactly 0, 1, 64, 65, T and T + 1 (T = LONG_ROW_SLOTS): an empty row, one slot, a
    full wave-load, one more, the longest row a wave sums alone and the shortest that is split."""
    check_operator(C, "degrees", dev)


@pytest.mark.parametrize("graph", G.SMALL_GRAPHS)
@pytest.mark.parametrize("C", G.SMALL_WIDTHS)
def test_graphs_of_one_two_three_nodes(dev, C, graph):
    check_operator(C, graph, dev)


def test_width_300_runs_as_column_blocks(dev):
    from rgb_experiment_amd import ops
    assert not ops.gine_supported(G.BLOCKED_WIDTH)
    check_operator(G.BLOCKED_WIDTH, "random", dev)


def test_aggregate_refusals(dev):
    from rgb_experiment_amd import ops
    _, n = G.graph_of("random")
    graph = operator_graph("random", dev)
    g = torch.Generator().manual_seed(3)
    rows = lambda r, w: torch.randn(r, w, generator=g).to(dev)
    nnz = graph.fwd.nnz
    assert not ops.gine_supported(67) and not ops.gine_supported(130)
    with pytest.raises(RuntimeError, match="pad the width"):
        ops.gine_aggregate(rows(n, 67), rows(nnz, 67), graph)
    with pytest.raises(RuntimeError, match="pad the width"):
        ops.gine_aggregate(rows(n, 256 + 67), rows(nnz, 256 + 67), graph)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.gine_aggregate(rows(n, 16), rows(nnz, 8), graph)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.gine_aggregate(rows(n, 8), rows(nnz - 1, 8), graph)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.gine_aggregate(rows(n - 1, 8), rows(nnz, 8), graph)
    with pytest.raises(RuntimeError, match="eps"):
        ops.gine_aggregate(rows(n, 8), rows(nnz, 8), graph, torch.zeros(2, device=dev))


def test_no_root_term_without_eps(dev):
    """eps=None: the bare sum; rows without in-edges store exact zeros."""
    from rgb_experiment_amd import ops
    graph = operator_graph("random", dev)
    x, e, cot, eps = device_case(40, "random", dev)
    with torch.no_grad():
        bare = ops.gine_aggregate(x, e, graph)
        full = ops.gine_aggregate(x, e, graph, eps)
    assert bare[:20].abs().max().item() == 0.0
    assert close(full - bare, (1 + G.EPS) * G.operator_case(40, "random")[0], FWD_TOL)


@pytest.mark.parametrize("graph", ["random", "powerlaw"])
def test_selective_passes(dev, graph):
    """Only x asks for a gradient: only gine_bwd_src is launched, and g_x has the bits of the full backward; only e:
    only gine_bwd_edge; eps alone: neither."""
    C = 40
    _, full = run_operator(C, graph, dev)
    for needs, launched in (((True, False, False), ["gine_fwd", "gine_bwd_src"]),
                            ((False, True, False), ["gine_fwd", "gine_bwd_edge"]),
                            ((False, False, True), ["gine_fwd"]),
                            ((True, True, True), ["gine_fwd", "gine_bwd_edge", "gine_bwd_src"])):
        sink = []
        _, got = run_operator(C, graph, dev, needs=needs, sink=sink)
        torch.cuda.synchronize()
        assert [str(kind) for kind, _, _ in sink if str(kind).startswith("gine")] == launched
        for need, a, b in zip(needs, got, full):
            assert (a is None) == (not need) and (a is None or torch.equal(a, b))


def test_two_runs_are_bit_identical(dev):
    """No float atomics and fixed summation orders: forward and backward twice on the hub-row graph, same bits."""
    (out_a, grads_a), (out_b, grads_b) = [run_operator(64, "powerlaw", dev) for _ in range(2)]
    assert torch.equal(out_a, out_b)
    for a, b in zip(grads_a, grads_b):
        assert torch.equal(a, b)


def test_strided_and_offset_operands(dev):
    """x and e as column blocks of wider matrices, a non-contiguous cotangent and an e view that starts off the 16-byte
    grid give the bits of separate contiguous operands."""
    from rgb_experiment_amd import ops
    C = 64
    graph = operator_graph("random", dev)
    x, e, cot, eps = device_case(C, "random", dev)

    def run(xv, ev, cotv):
        xv, ev = xv.detach().requires_grad_(True), ev.detach().requires_grad_(True)
        xs, es = (xv[:, 8:8 + C], ev[:, 4:4 + C]) if xv.size(1) > C else (xv, ev)
        out = ops.gine_aggregate(xs, es, graph, eps)
        (out * cotv).sum().backward()
        return out.detach(), (xv.grad[:, 8:8 + C], ev.grad[:, 4:4 + C]) if xv.size(1) > C else (xv.grad, ev.grad)

    plain_out, plain_grads = run(x, e, cot)
    pad = torch.nn.functional.pad
    wide_out, wide_grads = run(pad(x, (8, 8)), pad(e, (4, 12)), cot.t().contiguous().t())   # a column-major cotangent
    assert torch.equal(plain_out, wide_out)
    assert all(torch.equal(a, b) for a, b in zip(plain_grads, wide_grads))
    # an e that starts 4 bytes past a 16-byte boundary: the rows are read one float at a time (another lane layout, so
    # another order of the sums: compared at the tolerances; g_e has no sum in it and keeps its bits)
    flat = torch.zeros(e.numel() + 1, device=dev)
    flat[1:] = e.reshape(-1)
    off_grid = flat[1:].view_as(e)
    assert off_grid.data_ptr() % 16 == 4
    off_out, off_grads = run(x, off_grid, cot)
    assert close(off_out, plain_out.cpu().double(), FWD_TOL) and close(off_grads[0], plain_grads[0].cpu().double(), GRAD_TOL)
    assert torch.equal(off_grads[1], plain_grads[1])


def test_off_grid_view_at_a_width_that_needs_whole_vectors(dev):
    """C = 256 needs 16-byte rows: an e view 4 bytes off the grid is copied once (ops._rows_on_grid) and gives the bits of
    the aligned operand."""
    from rgb_experiment_amd import ops
    graph = operator_graph("random", dev)
    x, e, cot, eps = device_case(256, "random", dev)
    flat = torch.zeros(e.numel() + 1, device=dev)
    flat[1:] = e.reshape(-1)
    off_grid = flat[1:].view_as(e)
    assert off_grid.data_ptr() % 16 == 4
    outs = []
    for ev in (e, off_grid):
        ev = ev.detach().requires_grad_(True)
        out = ops.gine_aggregate(x, ev, graph, eps)
        (out * cot).sum().backward()
        outs.append((out.detach(), ev.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_edge_rows_to_slots_on_the_device(dev):
    """The permutation against edge_attr[perm], its cache, and the backward as the inverse gather."""
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_REMOVE_ADD, get_graph
    ei, n = G.graph_of("random")
    graph = operator_graph("random", dev)
    order = G.slots_of("random")[3].to(dev)
    g = torch.Generator().manual_seed(4)
    ea = torch.randn(ei.size(1), 5, generator=g).to(dev)
    got = ops.edge_rows_to_slots(ea, graph)
    assert torch.equal(got, ea[order]) and ops.edge_rows_to_slots(ea, graph) is got
    leaf = ea.clone().requires_grad_(True)
    cot = torch.randn(ei.size(1), 5, generator=g).to(dev)
    (ops.edge_rows_to_slots(leaf, graph) * cot).sum().backward()
    want = torch.empty_like(cot)
    want[order] = cot
    assert torch.equal(leaf.grad, want)
    with pytest.raises(RuntimeError, match="LOOPS_KEEP"):
        ops.edge_rows_to_slots(ea, get_graph(graph._keepalive, n, LOOPS_REMOVE_ADD))


# ---- layer ---------------------------------------------------------------------------------------------------------

def product_layer(ref, C, with_lin, train_eps, dev):
    from rgb_experiment_amd.nn import Linear
    import torch.nn as nn
    net = nn.Sequential(Linear(C, C), nn.ReLU(), Linear(C, 5))
    conv = GINEConv(net, eps=0.0, train_eps=train_eps, edge_dim=G.LAYER_F if with_lin else None)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return conv.to(dev)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("with_lin,train_eps", G.LAYER_FLAGS)
@pytest.mark.parametrize("C", G.LAYER_WIDTHS)
def test_layer_forward_backward(dev, C, with_lin, train_eps, train):
    """Output and the gradients of x, of edge_attr (it requires grad: the differentiable permutation runs) and of every
    parameter against the restatement; widths 67 and 130 are padded by the layer."""
    x, ei, ea, ref = G.layer_case(C, with_lin, train_eps)
    conv = product_layer(ref, C, with_lin, train_eps, dev).train(train)
    ref.train(train)
    assert (GINEConv.kernel_channels(C) != C) == (C in (67, 130))
    xd, ead = x.float().to(dev).requires_grad_(True), ea.float().to(dev).requires_grad_(True)
    out = conv(xd, ei.to(dev), ead)
    xr, ear = x.clone().requires_grad_(True), ea.clone().requires_grad_(True)
    want = ref(xr, ei, ear)
    assert out.shape == want.shape and finite(out) and close(out, want, FWD_TOL), "forward"
    cot = T.f32_exact(want.shape, torch.Generator().manual_seed(17))
    (out * cot.float().to(dev)).sum().backward()
    (want * cot).sum().backward()
    assert close(xd.grad, xr.grad, GRAD_TOL), "g_x"
    assert close(ead.grad, ear.grad, GRAD_TOL), "g_edge_attr"
    refp, got = dict(ref.named_parameters()), dict(conv.named_parameters())
    assert sorted(got) == sorted(refp) and ("eps" in got) == train_eps and ("lin.weight" in got) == with_lin
    for key, prm in got.items():
        assert prm.grad is not None and finite(prm.grad) and close(prm.grad, refp[key].grad, GRAD_TOL), key


def test_layer_with_static_edge_attr_caches_the_permutation(dev):
    """edge_attr without a gradient: permuted once, the second forward reuses the copy, same bits."""
    x, ei, ea, ref = G.layer_case(7, True, True)
    conv = product_layer(ref, 7, True, True, dev)
    xd, eid, ead = x.float().to(dev), ei.to(dev), ea.float().to(dev)
    with torch.no_grad():
        a, b = conv(xd, eid, ead), conv(xd, eid, ead)
    from rgb_experiment_amd.graph import LOOPS_KEEP, get_graph
    assert torch.equal(a, b) and len(get_graph(eid, xd.size(0), LOOPS_KEEP).__dict__["_edge_slots"]) == 1
    assert close(a, ref(x, ei, ea), FWD_TOL)


# ---- model, experiment() ----------------------------------------------------------------------------------------------

def test_model_against_restatement(dev):
    """Logits, `emb` and every parameter gradient of one training step (BatchNorm on batch statistics)."""
    x, y, ei, ea, model, ref = G.model_case()
    model.to(dev).train()
    ref.train()
    res = model(x.float().to(dev), ei.to(dev), ea.float().to(dev))
    want = ref(x, ei, ea)
    assert set(res.keys()) == {"out", "emb", "x"}
    assert close(res["emb"], want["emb"], FWD_TOL) and close(res["out"], want["out"], FWD_TOL)
    torch.nn.functional.nll_loss(res["out"], y.to(dev)).backward()
    torch.nn.functional.nll_loss(want["out"], y).backward()
    refp, got = dict(ref.named_parameters()), dict(model.named_parameters())
    assert sorted(got) == sorted(refp)
    for name, prm in got.items():
        assert prm.grad is not None and close(prm.grad, refp[name].grad, GRAD_TOL), name


def test_experiment_trains_and_hip_graph_equals_eager(dev):
    import rgb_experiment_amd as R
    n, f, c, d, epochs = 300, 16, 4, 6, 5
    gen = torch.Generator().manual_seed(11)
    ei = rand_graph(n, 1800, 13, loops=4, dups=4)
    data = R.Data(x=torch.randn(n, f, generator=gen), y=torch.randint(0, c, (n,), generator=gen), edge_index=ei,
                  edge_attr=torch.randn(ei.size(1), d, generator=gen))
    params = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0, "edge_dim": d}
    runs = []
    for graphed in (False, True):
        runs.append(R.experiment(params, specify_data=True, data=data, model_name="gine", learning_rate=0.01,
                                 epoch=epochs, need_to_reappear=True, print_print=False, return_model=True,
                                 use_hip_graph=graphed, implement_early_stopping=False, use_edge_attr=True))
    a, b = runs
    assert isinstance(a["model"], GINE)
    for key in ("ACC", "precision_score", "recall_score", "f1_macro", "f1_micro"):
        assert key in a and np.isfinite(float(a[key])), key
    assert b["used_hip_graph"] and not a["used_hip_graph"]
    assert len(a["history"]["train_loss"]) == epochs and len(b["history"]["train_loss"]) == epochs
    for key in ("train_loss", "val_loss", "test_loss"):                     # (the two loops divide the same sums on the
        assert np.allclose(a["history"][key], b["history"][key], rtol=0, atol=1e-6), key   # device and on the host)
    for key in ("train_acc", "val_acc", "test_acc"):
        assert a["history"][key] == b["history"][key], key
    sa, sb = a["model"].state_dict(), b["model"].state_dict()               # both loops train bit-identically
    assert sorted(sa) == sorted(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert a["history"]["train_loss"][-1] < a["history"]["train_loss"][0]
    for run in runs:                                                         # eps is trained, in both loops
        assert all(conv.eps.item() != 0.0 for conv in run["model"].convs)
    for ca, cb in zip(a["model"].convs, b["model"].convs):
        assert torch.equal(ca.eps, cb.eps)
    with pytest.raises(TypeError):                                           # flag off: the model's forward lacks its argument
        R.experiment(params, specify_data=True, data=data, model_name="gine", epoch=1, print_print=False,
                     use_hip_graph=False)
