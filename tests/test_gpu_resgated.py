"""ResGatedGraphConv on the MI355X: ops.resgated_aggregate (every vector width and group count of the lane layout, hub
rows, rows without in-edges, sources without out-edges, a graph without edges), gates saturated far beyond the range
of an unguarded expf, partial gradients, the inference form, ResGatedGraphConv, a seeded differential sweep of the
layer, the ResGatedGCN model and experiment(model_name="resgated") against the float64 restatement of
tests/test_resgated_host.py. The cases are that file's; it checks on the CPU that each is well-posed.

Tolerances are the project's for this depth of fp32 gather (tests/test_gpu_transformer.py): forward
1e-4 * max(1, |ref|max), gradients 2e-4 * max(1, |ref|max). Every element is compared.

Rows the kernels have no slot for. The op allocates its output and its gradients with torch.empty. Before every operator
call the allocator's free blocks of that size are filled with NaN (`poison`), so a row that a kernel skipped shows as
NaN in the comparison instead of passing on stale zeros; `finite` is asserted on top."""
import copy
import functools

import numpy as np
import pytest
import torch

import test_resgated_host as RG
import test_transformer_host as T
from test_gpu_ggnn import close, rand_graph
from test_gpu_transformer import device_graph, finite, poison
from test_resgated_host import ResGatedGCN, ResGatedGraphConv

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = T.FWD_TOL, T.GRAD_TOL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def operator_graph(name, dev):
    """The device graph of a host-file graph, with what the cases rely on asserted once."""
    ei, n = T.graph_of(name)
    graph = device_graph(ei, n, dev)
    assert graph.fwd.nnz == ei.size(1) and graph.bwd.nnz == ei.size(1)        # nothing added, nothing coalesced
    if name == "random":
        indeg = (graph.fwd.rowptr[1:] - graph.fwd.rowptr[:-1]).cpu()
        outdeg = (graph.bwd.rowptr[1:] - graph.bwd.rowptr[:-1]).cpu()
        assert bool((indeg[:20] == 0).all()) and bool((outdeg[20:40] == 0).all())
    if name == "powerlaw":
        assert graph.fwd.split is not None and graph.bwd.split is not None    # both chunk paths run
    if name == "no_edges":
        assert graph.fwd.nnz == 0
    return graph


def run_operator(C, graph_name, dev, saturated=False, needs=(True, True, True)):
    """ops.resgated_aggregate forward and the gradients asked for (`needs`: of k, q, v); -> (out, [g_k, g_q, g_v])."""
    from rgb_experiment_amd import ops
    _, n = T.graph_of(graph_name)
    graph = operator_graph(graph_name, dev)
    case = RG.operator_case(C, graph_name, saturated)
    k_d, q_d, v_d = (t.float().to(dev).requires_grad_(need) for t, need in zip(case[:3], needs))
    cot_d = case[3].float().to(dev)
    poison(dev, (n, C))
    out = ops.resgated_aggregate(k_d, q_d, v_d, graph)
    (out * cot_d).sum().backward()
    return out.detach(), [k_d.grad, q_d.grad, v_d.grad]


def check_operator(C, graph_name, dev, saturated=False):
    out, grads = run_operator(C, graph_name, dev, saturated)
    assert finite(out, *grads), "a row was left unwritten, or a gate overflowed"
    want = RG.reference(C, graph_name, saturated)
    assert close(out, want[0], FWD_TOL), "forward"
    for name, got, ref in zip(RG.NAMES[1:], grads, want[1]):
        assert close(got, ref, GRAD_TOL), name
    if graph_name == "no_edges":  # exact zeros, not small numbers
        for t in [out] + grads:
            assert t.abs().max().item() == 0.0
    if graph_name == "random":    # rows without in-edges / sources without out-edges: exact zeros
        assert out[:20].abs().max().item() == 0.0 and grads[0][:20].abs().max().item() == 0.0
        assert grads[1][20:40].abs().max().item() == 0.0 and grads[2][20:40].abs().max().item() == 0.0
    return out, grads


@pytest.mark.parametrize("graph", RG.GRAPH_NAMES)
@pytest.mark.parametrize("C", RG.WIDTHS)
def test_aggregate_forward_backward(dev, C, graph):
    from rgb_experiment_amd import ops
    assert ops.resgated_supported(C)
    check_operator(C, graph, dev)


@pytest.mark.parametrize("graph", RG.SATURATED_GRAPHS)
@pytest.mark.parametrize("C", RG.SATURATED_WIDTHS)
def test_aggregate_saturated_gates(dev, C, graph):
    """k, q of standard deviation 128 (|k_i + q_j| up to ~900, three quarters of the gates exactly 0 or 1:
    tests/test_resgated_host.py asserts it), at the unchanged tolerances."""
    check_operator(C, graph, dev, saturated=True)


def test_aggregate_refusals(dev):
    from rgb_experiment_amd import ops
    _, n = T.graph_of("random")
    graph = operator_graph("random", dev)
    g = torch.Generator().manual_seed(3)
    wide = lambda w: torch.randn(n, w, generator=g).to(dev)
    assert not ops.resgated_supported(67) and not ops.resgated_supported(130)
    with pytest.raises(RuntimeError, match="pad the width"):
        ops.resgated_aggregate(wide(67), wide(67), wide(67), graph)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.resgated_aggregate(wide(16), wide(16), wide(8), graph)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.resgated_aggregate(wide(8)[:5], wide(8)[:5], wide(8)[:5], graph)


@pytest.mark.parametrize("graph", ["random", "powerlaw"])
def test_partial_gradients(dev, graph):
    """Only k asks for a gradient: the source pass is skipped (q.grad and v.grad stay None) and g_k has the bits of the
    full backward; the same the other way round, and with q or v alone."""
    C = 40
    _, full = run_operator(C, graph, dev)
    _, only_k = run_operator(C, graph, dev, needs=(True, False, False))
    assert only_k[1] is None and only_k[2] is None and torch.equal(only_k[0], full[0])
    _, only_src = run_operator(C, graph, dev, needs=(False, True, True))
    assert only_src[0] is None and torch.equal(only_src[1], full[1]) and torch.equal(only_src[2], full[2])
    _, only_q = run_operator(C, graph, dev, needs=(False, True, False))
    assert only_q[0] is None and only_q[2] is None and torch.equal(only_q[1], full[1])
    _, only_v = run_operator(C, graph, dev, needs=(False, False, True))
    assert only_v[0] is None and only_v[1] is None and torch.equal(only_v[2], full[2])


def test_partial_gradients_skip_the_other_pass(dev):
    """Counted at the entry points' timing labels: k alone runs no source pass, q alone no target pass."""
    from rgb_experiment_amd import ops
    graph = operator_graph("random", dev)
    case = RG.operator_case(8, "random")
    for needs, want in (((True, False, False), ["resgated_fwd", "resgated_bwd_dst"]),
                        ((False, True, False), ["resgated_fwd", "resgated_bwd_src"]),
                        ((True, True, True), ["resgated_fwd", "resgated_bwd_dst", "resgated_bwd_src"])):
        k, q, v = (t.float().to(dev).requires_grad_(need) for t, need in zip(case[:3], needs))
        sink = []
        ops.set_event_sink(sink)
        try:
            ops.resgated_aggregate(k, q, v, graph).sum().backward()
        finally:
            ops.set_event_sink(None)
        torch.cuda.synchronize()
        assert [str(kind) for kind, _, _ in sink if str(kind).startswith("resgated")] == want


@pytest.mark.parametrize("graph", ["random", "powerlaw"])
def test_inference_form_stores_the_same_bits(dev, graph):
    from rgb_experiment_amd import ops
    g = operator_graph(graph, dev)
    k, q, v = (t.float().to(dev) for t in RG.operator_case(40, graph)[:3])
    with torch.no_grad():
        plain = ops.resgated_aggregate(k, q, v, g)
    saved = ops.resgated_aggregate(k.clone().requires_grad_(True), q, v, g)
    assert saved.grad_fn is not None and plain.grad_fn is None
    assert torch.equal(plain, saved.detach())


def test_two_runs_are_bit_identical(dev):
    """No float atomics and fixed summation orders: forward and backward twice on the hub-row graph, same bits."""
    (out_a, grads_a), (out_b, grads_b) = [run_operator(64, "powerlaw", dev) for _ in range(2)]
    assert torch.equal(out_a, out_b)
    for a, b in zip(grads_a, grads_b):
        assert torch.equal(a, b)


def test_column_blocks_of_one_product_are_taken_as_they_are(dev):
    """k | q | v as views into one [n, 3C + 8] matrix (what the layer hands over) give the bits of three separate
    matrices."""
    from rgb_experiment_amd import ops
    C = 64
    graph = operator_graph("random", dev)
    k, q, v = (t.float().to(dev) for t in RG.operator_case(C, "random")[:3])
    h = torch.cat([k, q, v, torch.zeros(k.size(0), 8, device=dev)], dim=1)
    with torch.no_grad():
        apart = ops.resgated_aggregate(k, q, v, graph)
        views = ops.resgated_aggregate(h[:, :C], h[:, C:2 * C], h[:, 2 * C:3 * C], graph)
    assert torch.equal(apart, views)


# ---- layer ---------------------------------------------------------------------------------------------------------

def compare_layer(conv, ref, x, ei, dev, cot_seed=17):
    """Output and the gradients of x and of every parameter of the layer `conv` (on the device) against `ref`."""
    xd = x.float().to(dev).requires_grad_(True)
    out = conv(xd, ei.to(dev))
    xr = x.clone().requires_grad_(True)
    want = ref(xr, ei)
    assert out.shape == want.shape and finite(out) and close(out, want, FWD_TOL), "forward"
    cot = T.f32_exact(want.shape, torch.Generator().manual_seed(cot_seed))
    (out * cot.float().to(dev)).sum().backward()
    (want * cot).sum().backward()
    assert close(xd.grad, xr.grad, GRAD_TOL), "g_x"
    refp, got = dict(ref.named_parameters()), dict(conv.named_parameters())
    assert sorted(got) == sorted(refp)
    for key, prm in got.items():
        assert prm.grad is not None and finite(prm.grad) and close(prm.grad, refp[key].grad, GRAD_TOL), key


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("root_weight,bias", RG.LAYER_FLAGS)
@pytest.mark.parametrize("C", RG.LAYER_WIDTHS)
def test_layer_forward_backward(dev, C, root_weight, bias, train):
    from rgb_experiment_amd.nn import GATConv
    x, ei, ref = RG.layer_case(C, root_weight, bias)
    conv = ResGatedGraphConv(RG.LAYER_F, C, root_weight=root_weight, bias=bias)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    conv.to(dev).train(train)
    ref.train(train)
    assert (GATConv.kernel_channels(C) != C) == (C in (67, 130))
    compare_layer(conv, ref, x, ei, dev)


SWEEP_SEEDS = list(range(24))


def sweep_case(seed):
    """One draw of the sweep: n in [1, 300], E in [0, 8 n], input width in [1, 40], C in [1, 140], root_weight, bias;
    edges uniform over the node pairs (self-loops and duplicates as they fall), x ~ N(0, 1), parameters as in
    tests/test_resgated_host.layer_case. -> (shape dict, x, edge_index, reference layer)."""
    g = torch.Generator().manual_seed(77000 + seed)
    draw = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    n = draw(1, 300)
    shape = dict(n=n, E=draw(0, 8 * n), f=draw(1, 40), C=draw(1, 140), root_weight=bool(draw(0, 1)), bias=bool(draw(0, 1)))
    ei = torch.randint(0, n, (2, shape["E"]), generator=g)
    x = T.f32_exact((n, shape["f"]), g)
    ref = RG.RefResGatedGraphConv(shape["f"], shape["C"], root_weight=shape["root_weight"], bias=shape["bias"])
    with torch.no_grad():
        for key, prm in ref.named_parameters():
            prm.copy_(T.f32_exact(prm.shape, g, prm.size(-1) ** -0.5 if key.endswith("weight") else 0.5))
    return shape, x, ei, ref


@pytest.mark.parametrize("seed", SWEEP_SEEDS)
def test_layer_sweep(dev, seed):
    """The layer forward and backward against the restatement on a drawn shape; the draw is checked for well-posedness
    first (float32 on the CPU, reversed edge order, a quarter of the tolerance)."""
    shape, x, ei, ref = sweep_case(seed)
    print(shape)
    low = copy.deepcopy(ref).float()
    with torch.no_grad():
        assert T.share_of_tolerance(low(x.float(), ei, reverse=True), ref(x, ei), FWD_TOL) <= T.WELL_POSED_SHARE
    conv = ResGatedGraphConv(shape["f"], shape["C"], root_weight=shape["root_weight"], bias=shape["bias"])
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    compare_layer(conv.to(dev), ref, x, ei, dev, cot_seed=seed)


def test_sweep_draws_cover_the_space():
    shapes = [sweep_case(s)[0] for s in SWEEP_SEEDS]
    from rgb_experiment_amd.nn import GATConv
    assert {s["root_weight"] for s in shapes} == {True, False} and {s["bias"] for s in shapes} == {True, False}
    assert any(GATConv.kernel_channels(s["C"]) != s["C"] for s in shapes)          # padded widths
    assert any(s["C"] > 128 for s in shapes) and any(s["C"] <= 16 for s in shapes)
    assert any(s["C"] % 2 == 1 for s in shapes) and any(s["C"] % 4 == 0 for s in shapes)


# ---- model, experiment() ----------------------------------------------------------------------------------------------

def test_model_against_restatement(dev):
    """Logits, `emb` and every parameter gradient of one training step (BatchNorm on batch statistics)."""
    x, y, ei, model, ref = RG.model_case()
    model.to(dev).train()
    ref.train()
    res = model(x.float().to(dev), ei.to(dev))
    want = ref(x, ei)
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
    n, f, c, epochs = 300, 16, 4, 5
    gen = torch.Generator().manual_seed(11)
    ei = rand_graph(n, 1800, 13, loops=4, dups=4)
    data = R.Data(x=torch.randn(n, f, generator=gen), y=torch.randint(0, c, (n,), generator=gen), edge_index=ei)
    params = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0}
    runs = []
    for graphed in (False, True):
        runs.append(R.experiment(params, specify_data=True, data=data, model_name="resgated", learning_rate=0.01,
                                 epoch=epochs, need_to_reappear=True, print_print=False, return_model=True,
                                 use_hip_graph=graphed, implement_early_stopping=False))
    a, b = runs
    assert isinstance(a["model"], ResGatedGCN)
    for key in ("ACC", "precision_score", "recall_score", "f1_macro", "f1_micro"):
        assert key in a and np.isfinite(float(a[key])), key
    assert b["used_hip_graph"] and not a["used_hip_graph"]
    assert len(a["history"]["train_loss"]) == epochs and len(b["history"]["train_loss"]) == epochs
    for key in ("train_loss", "val_loss", "test_loss"):
        assert np.allclose(a["history"][key], b["history"][key], rtol=0, atol=1e-6), key
    for key in ("train_acc", "val_acc", "test_acc"):
        assert a["history"][key] == b["history"][key], key
