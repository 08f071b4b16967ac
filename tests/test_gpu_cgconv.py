"""CGConv on the MI355X: ops.cgconv_aggregate (every vector width and group count of the lane layout, hub rows in both
CSRs, rows of exactly 0 / 1 / 64 / 65 / T / T + 1 slots, rows without in-edges, sources without out-edges, graphs of one
to three nodes, a graph without edges, with and without the edge term, add and mean, saturated arguments), selective
backward passes, bit-identical runs, strided and offset operands, CGConv, the CGCNN model and
experiment(model_name="cgcnn", use_edge_attr=True) against the float64 restatement of tests/test_cgconv_host.py. The
cases are that file's; it checks on the CPU that each is well-posed. PyG is not importable here: parity unpinned.

Tolerances are the project's for this depth of fp32 gather (tests/test_gpu_transformer.py): forward
1e-4 * max(1, |ref|max), gradients 2e-4 * max(1, |ref|max). Every element is compared.

Rows the kernels have no slot for. The op allocates its output and its gradients with torch.empty. Before every operator
call the allocator's free blocks of those sizes ([N, C], [N, 2C] and [E, 2C]) are filled with NaN (`poison`), so a row
or a slot that a kernel skipped shows as NaN in the comparison instead of passing on stale zeros; `finite` is asserted
on top."""
import functools
import itertools

import numpy as np
import pytest
import torch

import test_cgconv_host as H
import test_transformer_host as T
from test_gpu_ggnn import close, rand_graph
from test_gpu_transformer import device_graph, finite, poison
from test_cgconv_host import CGCNN, CGConv

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = T.FWD_TOL, T.GRAD_TOL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def operator_graph(name, dev):
    """The device graph of a host-file graph, with what the cases rely on asserted once."""
    ei, n = H.any_graph_of(name)
    graph = device_graph(ei, n, dev)
    assert graph.fwd.nnz == ei.size(1) and graph.bwd.nnz == ei.size(1)        # nothing added, nothing coalesced
    indeg = (graph.fwd.rowptr[1:] - graph.fwd.rowptr[:-1]).cpu()
    outdeg = (graph.bwd.rowptr[1:] - graph.bwd.rowptr[:-1]).cpu()
    if ei.size(1):   # slot p of the device's CSR is edge order[p] of the host file
        assert torch.equal(graph.fwd.perm[:graph.fwd.nnz].cpu().long(), H.any_slots_of(name)[3])
    if name == "random":
        assert bool((indeg[:20] == 0).all()) and bool((outdeg[20:40] == 0).all())
    if name == "powerlaw":
        assert graph.fwd.split is not None and graph.bwd.split is not None    # both chunk paths run
    if name == "degrees":   # exactly one row beyond the threshold in each CSR: T stays whole, T + 1 is split
        assert tuple(indeg[:6].tolist()) == H.G.DEGREES and tuple(outdeg[6:12].tolist()) == H.G.DEGREES
        assert graph.fwd.split["n_long"] == 1 and graph.bwd.split["n_long"] == 1
    if name == "no_edges":
        assert graph.fwd.nnz == 0
    return graph


def device_case(C, graph_name, dim, dev, saturated=False):
    """(a, b, c_slot or None, root, cot) of a host-file case on the device: c in forward CSR slot order."""
    a, b, c, root, cot = H.operator_case(C, graph_name, dim, saturated)
    order = H.any_slots_of(graph_name)[3]
    put = lambda t: t.float().to(dev)
    return put(a), put(b), None if c is None else put(c[order]), put(root), put(cot)


def run_operator(C, graph_name, dim, aggr, dev, needs=(True, True, True, True), sink=None, saturated=False):
    """ops.cgconv_aggregate forward and the gradients asked for (`needs`: of a, b, c_slot, root);
    -> (out, [g_a, g_b, g_c, g_root]), g_c in forward CSR slot order (None with dim = 0)."""
    from rgb_experiment_amd import ops
    ei, n = H.any_graph_of(graph_name)
    graph = operator_graph(graph_name, dev)
    a, b, c, root, cot = device_case(C, graph_name, dim, dev, saturated)
    leaves = [None if t is None else t.requires_grad_(need) for t, need in zip((a, b, c, root), needs)]
    poison(dev, (n, C), (n, 2 * C), (max(ei.size(1), 1), 2 * C))
    if sink is not None:
        ops.set_event_sink(sink)
    try:
        out = ops.cgconv_aggregate(leaves[0], leaves[1], leaves[2], graph, C, aggr, root=leaves[3])
        (out * cot).sum().backward()
    finally:
        ops.set_event_sink(None)
    return out.detach(), [None if t is None else t.grad for t in leaves]


def check_operator(C, graph_name, dim, aggr, dev, saturated=False):
    out, grads = run_operator(C, graph_name, dim, aggr, dev, saturated=saturated)
    assert finite(out, *[g for g in grads if g is not None]), "a row or a slot was left unwritten"
    want = H.reference(C, graph_name, dim, aggr, saturated)
    a, b, c, root, cot = H.operator_case(C, graph_name, dim, saturated)
    ei, n = H.any_graph_of(graph_name)
    order = H.any_slots_of(graph_name)[3]
    assert out.shape == (n, C) and close(out, want[0], FWD_TOL), "forward"
    assert grads[0].shape == (n, 2 * C) and close(grads[0], want[1][0], GRAD_TOL), "g_a"
    assert grads[1].shape == (n, 2 * C) and close(grads[1], want[1][1], GRAD_TOL), "g_b"
    assert (grads[2] is None) == (dim == 0)
    if dim:
        assert grads[2].shape == (ei.size(1), 2 * C)
        if ei.size(1):
            assert close(grads[2], want[1][2][order], GRAD_TOL), "g_c"
    assert torch.equal(grads[3].cpu(), cot.float()), "g_root = gout"
    if graph_name == "no_edges":  # exact: the root term alone, and zero gradients
        assert torch.equal(out.cpu(), root.float())
        assert grads[0].abs().max().item() == 0.0 and grads[1].abs().max().item() == 0.0
    if graph_name == "random":    # rows without in-edges / sources without out-edges
        assert torch.equal(out[:20].cpu(), root.float()[:20]) and grads[0][:20].abs().max().item() == 0.0
        assert grads[1][20:40].abs().max().item() == 0.0
    return out, grads


@pytest.mark.parametrize("aggr", H.AGGRS)
@pytest.mark.parametrize("dim", H.DIMS)
@pytest.mark.parametrize("graph", H.GRAPH_NAMES)
@pytest.mark.parametrize("C", H.WIDTHS)
def test_aggregate_forward_backward(dev, C, graph, dim, aggr):
    from rgb_experiment_amd import ops
    assert ops.cgconv_supported(C)
    check_operator(C, graph, dim, aggr, dev)


@pytest.mark.parametrize("aggr", H.AGGRS)
@pytest.mark.parametrize("dim", H.DIMS)
@pytest.mark.parametrize("graph", H.SATURATED_GRAPHS)
@pytest.mark.parametrize("C", H.SATURATED_WIDTHS)
def test_saturated_arguments(dev, C, graph, dim, aggr):
    """a, b, c of standard deviation 128: arguments in the hundreds in both branches, most gates exactly 0 or 1; finite,
    at the unchanged tolerances."""
    check_operator(C, graph, dim, aggr, dev, saturated=True)


@pytest.mark.parametrize("aggr", H.AGGRS)
@pytest.mark.parametrize("dim", H.DIMS)
@pytest.mark.parametrize("C", H.DEGREE_WIDTHS)
def test_rows_of_exact_lengths(dev, C, dim, aggr):
    """In-degrees and out-degrees of exactly 0, 1, 64, 65, T and T + 1 (T = LONG_ROW_SLOTS): an empty row, one slot, a
    full wave-load, one more, the longest row a wave sums alone and the shortest that is split."""
    check_operator(C, "degrees", dim, aggr, dev)


@pytest.mark.parametrize("aggr", H.AGGRS)
@pytest.mark.parametrize("graph", H.SMALL_GRAPHS)
@pytest.mark.parametrize("C", H.SMALL_WIDTHS)
def test_graphs_of_one_two_three_nodes(dev, C, graph, aggr):
    check_operator(C, graph, 5, aggr, dev)


def test_no_root_term(dev):
    """root=None: the bare aggregate; rows without in-edges store exact zeros."""
    from rgb_experiment_amd import ops
    graph = operator_graph("random", dev)
    a, b, c, root, cot = device_case(40, "random", 5, dev)
    for aggr in H.AGGRS:
        poison(dev, (a.size(0), 40))
        with torch.no_grad():
            bare = ops.cgconv_aggregate(a, b, c, graph, 40, aggr)
            full = ops.cgconv_aggregate(a, b, c, graph, 40, aggr, root=root)
        assert finite(bare) and bare[:20].abs().max().item() == 0.0
        assert close(full - bare, H.operator_case(40, "random", 5)[3], FWD_TOL)


def test_aggregate_refusals(dev):
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_REMOVE_ADD, get_graph
    _, n = H.any_graph_of("random")
    graph = operator_graph("random", dev)
    g = torch.Generator().manual_seed(3)
    rows = lambda r, w: torch.randn(r, w, generator=g).to(dev)
    nnz = graph.fwd.nnz
    assert not ops.cgconv_supported(67) and not ops.cgconv_supported(130)
    with pytest.raises(RuntimeError, match="pad the width"):
        ops.cgconv_aggregate(rows(n, 134), rows(n, 134), None, graph, 67)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.cgconv_aggregate(rows(n, 16), rows(n, 8), None, graph, 8)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.cgconv_aggregate(rows(n, 8), rows(n, 8), None, graph, 8)             # rows hold both halves: [N, 2C]
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.cgconv_aggregate(rows(n, 16), rows(n, 16), rows(nnz - 1, 16), graph, 8)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.cgconv_aggregate(rows(n, 16), rows(n, 16), rows(nnz, 8), graph, 8)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.cgconv_aggregate(rows(n, 16), rows(n, 16), None, graph, 8, root=rows(n, 16))
    with pytest.raises(NotImplementedError, match="aggr"):
        ops.cgconv_aggregate(rows(n, 16), rows(n, 16), None, graph, 8, "max")
    with pytest.raises(RuntimeError, match="LOOPS_KEEP"):
        ops.cgconv_aggregate(rows(n, 16), rows(n, 16), None, get_graph(graph._keepalive, n, LOOPS_REMOVE_ADD), 8)


@pytest.mark.parametrize("graph", ["random", "powerlaw"])
def test_selective_passes(dev, graph):
    """Every subset of requires_grad on a / b / c (root always asks, so that a backward runs): the target-side pass is
    launched only if a or c asks, the source-side pass only if b does, and every gradient has the bits of the full
    backward."""
    C, dim, aggr = 40, 5, "mean"
    _, full = run_operator(C, graph, dim, aggr, dev)
    for needs in itertools.product((False, True), repeat=3):
        launched = ["cgconv_fwd"] + ["cgconv_bwd_dst"] * (needs[0] or needs[2]) + ["cgconv_bwd_src"] * needs[1]
        sink = []
        _, got = run_operator(C, graph, dim, aggr, dev, needs=needs + (True,), sink=sink)
        torch.cuda.synchronize()
        assert [str(kind) for kind, _, _ in sink if str(kind).startswith("cgconv")] == launched, needs
        for need, p, q in zip(needs + (True,), got, full):
            assert (p is None) == (not need) and (p is None or (finite(p) and torch.equal(p, q))), needs


@pytest.mark.parametrize("dim", H.DIMS)
def test_two_runs_are_bit_identical(dev, dim):
    """No float atomics and fixed summation orders: forward and backward twice on the hub-row graph, same bits."""
    (out_a, grads_a), (out_b, grads_b) = [run_operator(64, "powerlaw", dim, "add", dev) for _ in range(2)]
    assert torch.equal(out_a, out_b)
    for p, q in zip(grads_a, grads_b):
        assert (p is None) == (q is None) and (p is None or torch.equal(p, q))


def test_strided_and_offset_operands(dev):
    """a and b as the column blocks of ONE wider matrix (as the layer hands them), c and root as column blocks of wider
    matrices and a non-contiguous cotangent give the bits of separate contiguous operands; a c view that starts off the
    16-byte grid is read one float at a time (another lane layout, so another order of the sums: compared at the
    tolerances)."""
    from rgb_experiment_amd import ops
    C = 64
    graph = operator_graph("random", dev)
    a, b, c, root, cot = device_case(C, "random", 5, dev)
    pad = torch.nn.functional.pad

    def run(av, bv, cv, rv, cotv):
        leaves = [t.detach().requires_grad_(True) for t in (av, bv, cv, rv)]
        out = ops.cgconv_aggregate(*leaves[:3], graph, C, "mean", root=leaves[3])
        (out * cotv).sum().backward()
        return out.detach(), [t.grad for t in leaves]

    plain_out, plain = run(a, b, c, root, cot)
    h = pad(torch.cat([a, b], dim=1), (8, 4)).requires_grad_(True)           # [n, 8 + 4C + 4]
    cw = pad(c, (4, 12)).requires_grad_(True)
    rw = pad(root, (12, 4)).requires_grad_(True)
    out = ops.cgconv_aggregate(h[:, 8:8 + 2 * C], h[:, 8 + 2 * C:8 + 4 * C], cw[:, 4:4 + 2 * C], graph, C, "mean",
                               root=rw[:, 12:12 + C])
    (out * cot.t().contiguous().t()).sum().backward()                        # a column-major cotangent
    assert torch.equal(out.detach(), plain_out)
    assert torch.equal(h.grad[:, 8:8 + 2 * C], plain[0]) and torch.equal(h.grad[:, 8 + 2 * C:8 + 4 * C], plain[1])
    assert torch.equal(cw.grad[:, 4:4 + 2 * C], plain[2]) and torch.equal(rw.grad[:, 12:12 + C], plain[3])
    assert h.grad[:, :8].abs().max().item() == 0.0 and cw.grad[:, :4].abs().max().item() == 0.0
    flat = torch.zeros(c.numel() + 1, device=dev)
    flat[1:] = c.reshape(-1)
    off_grid = flat[1:].view_as(c)
    assert off_grid.data_ptr() % 16 == 4
    off_out, off = run(a, b, off_grid, root, cot)
    assert close(off_out, plain_out.cpu().double(), FWD_TOL)
    for p, q in zip(off[:3], plain[:3]):
        assert finite(p) and close(p, q.cpu().double(), GRAD_TOL)


def test_off_grid_view_at_a_width_that_needs_whole_vectors(dev):
    """C = 256 needs 16-byte rows: a c view 4 bytes off the grid is copied once (ops._rows_on_grid) and gives the bits of
    the aligned operand."""
    from rgb_experiment_amd import ops
    graph = operator_graph("random", dev)
    a, b, c, root, cot = device_case(256, "random", 5, dev)
    flat = torch.zeros(c.numel() + 1, device=dev)
    flat[1:] = c.reshape(-1)
    off_grid = flat[1:].view_as(c)
    assert off_grid.data_ptr() % 16 == 4
    outs = []
    for cv in (c, off_grid):
        cv, av = cv.detach().requires_grad_(True), a.detach().requires_grad_(True)
        out = ops.cgconv_aggregate(av, b, cv, graph, 256, "add", root=root)
        (out * cot).sum().backward()
        outs.append((out.detach(), cv.grad, av.grad))
    assert all(torch.equal(p, q) for p, q in zip(*outs))


# ---- layer ---------------------------------------------------------------------------------------------------------

def product_layer(ref, C, dim, batch_norm, aggr, dev):
    conv = CGConv(C, dim=dim, aggr=aggr, batch_norm=batch_norm)
    conv.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()}, strict=True)
    return conv.to(dev)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("dim,batch_norm,aggr", H.LAYER_FLAGS)
@pytest.mark.parametrize("C", H.LAYER_WIDTHS)
def test_layer_forward_backward(dev, C, dim, batch_norm, aggr, train):
    """Output and the gradients of x, of edge_attr (it requires grad: the differentiable permutation runs) and of every
    parameter against the restatement; widths 67 and 130 are padded by the layer; with batch_norm the root term is
    dense work, without it (and without padding) it runs in the kernel."""
    from rgb_experiment_amd.nn import GATConv
    x, ei, ea, ref = H.layer_case(C, dim, batch_norm, aggr)
    conv = product_layer(ref, C, dim, batch_norm, aggr, dev).train(train)
    ref.train(train)
    assert (GATConv.kernel_channels(C) != C) == (C in (67, 130))
    xd = x.float().to(dev).requires_grad_(True)
    ead = None if ea is None else ea.float().to(dev).requires_grad_(True)
    out = conv(xd, ei.to(dev), ead) if dim else conv(xd, ei.to(dev))
    xr = x.clone().requires_grad_(True)
    ear = None if ea is None else ea.clone().requires_grad_(True)
    want = ref(xr, ei, ear)
    assert out.shape == want.shape and finite(out) and close(out, want, FWD_TOL), "forward"
    cot = T.f32_exact(want.shape, torch.Generator().manual_seed(17))
    (out * cot.float().to(dev)).sum().backward()
    (want * cot).sum().backward()
    assert close(xd.grad, xr.grad, GRAD_TOL), "g_x"
    if dim:
        assert close(ead.grad, ear.grad, GRAD_TOL), "g_edge_attr"
    refp, got = dict(ref.named_parameters()), dict(conv.named_parameters())
    assert sorted(got) == sorted(refp) and ("bn.weight" in got) == batch_norm and len(got) == 4 + 2 * batch_norm
    for key, prm in got.items():
        assert prm.grad is not None and finite(prm.grad) and close(prm.grad, refp[key].grad, GRAD_TOL), key
    if batch_norm and train:
        assert close(conv.bn.running_mean, ref.bn.running_mean, FWD_TOL)
        assert close(conv.bn.running_var, ref.bn.running_var, FWD_TOL)


def test_layer_without_bias_and_without_edges(dev):
    """bias=False (no bias rows in the product) and an empty edge list with dim > 0 (no slot, no edge product): x alone."""
    x, ei, ea, ref = H.layer_case(7, 6, False, "add")
    nobias = H.RefCGConv(7, 6, "add", False, bias=False)
    nobias.load_state_dict({k: v for k, v in ref.state_dict().items() if not k.endswith("bias")}, strict=True)
    conv = CGConv(7, dim=6, bias=False)
    conv.load_state_dict({k: v.float() for k, v in nobias.state_dict().items()}, strict=True)
    conv.to(dev)
    xd, ead = x.float().to(dev), ea.float().to(dev)
    assert close(conv(xd, ei.to(dev), ead), nobias(x, ei, ea), FWD_TOL)
    empty = torch.zeros((2, 0), dtype=torch.int64, device=dev)
    assert torch.equal(conv(xd, empty, ead[:0]), xd)


# ---- model, experiment() ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge_dim", H.MODEL_EDGE_DIMS)
def test_model_against_restatement(dev, edge_dim):
    """Logits, `emb` and every parameter gradient of one training step (BatchNorm on batch statistics)."""
    x, y, ei, ea, model, ref = H.model_case(edge_dim)
    model.to(dev).train()
    ref.train()
    res = model(x.float().to(dev), ei.to(dev), None if ea is None else ea.float().to(dev))
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
        runs.append(R.experiment(params, specify_data=True, data=data, model_name="cgcnn", learning_rate=0.01,
                                 epoch=epochs, need_to_reappear=True, print_print=False, return_model=True,
                                 use_hip_graph=graphed, implement_early_stopping=False, use_edge_attr=True))
    a, b = runs
    assert isinstance(a["model"], CGCNN)
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
    with pytest.raises(ValueError, match="edge_attr"):                       # flag off: the layers miss their rows
        R.experiment(params, specify_data=True, data=data, model_name="cgcnn", epoch=1, print_print=False,
                     use_hip_graph=False)
    plain = R.experiment({"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0}, specify_data=True, data=data,
                         model_name="cgcnn", learning_rate=0.01, epoch=epochs, need_to_reappear=True, print_print=False,
                         return_model=True, use_hip_graph=False, implement_early_stopping=False)
    assert all(conv.dim == 0 for conv in plain["model"].convs)               # edge_dim = 0: an ordinary graph, no flag
    assert plain["history"]["train_loss"][-1] < plain["history"]["train_loss"][0]
