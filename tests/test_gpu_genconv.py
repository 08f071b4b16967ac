"""GENConv / DeeperGCN on the MI355X: ops.softmax_aggregate (every vector width and group count of the lane layout, hub
rows on both CSRs, rows without in-edges, sources without out-edges, a graph without edges; one temperature and one per
channel, negative ones included), scores far beyond the range of an unguarded expf, the inference form, partial
gradients, GENConv, a seeded differential sweep of the layer, the DeeperGCN model and
experiment(model_name="deepergcn") against the float64 restatement of tests/test_genconv_host.py. The cases are that
file's; it checks on the CPU that each is well-posed.

Tolerances are the project's for this depth of fp32 gather (tests/test_gpu_transformer.py): forward
1e-4 * max(1, |ref|max), gradients 2e-4 * max(1, |ref|max). Every element is compared.

Rows the kernels have no slot for. The op allocates its outputs with torch.empty. Before every operator call the
allocator's free blocks of that size are filled with NaN (`poison`), so a row that a kernel skipped shows as NaN in the
comparison instead of passing on stale zeros; `finite` is asserted on top."""
import copy
import functools

import numpy as np
import pytest
import torch

import test_genconv_host as GH
import test_transformer_host as T
from test_gpu_ggnn import close, rand_graph
from test_gpu_transformer import device_graph, finite, poison
from test_genconv_host import DeeperGCN, GENConv

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


def run_operator(C, graph_name, kind, dev, needs=(True, True)):
    """ops.softmax_aggregate forward and the gradients asked for (`needs`: of m, t); -> (out, [g_m, g_t])."""
    from rgb_experiment_amd import ops
    _, n = T.graph_of(graph_name)
    graph = operator_graph(graph_name, dev)
    case = GH.operator_case(C, graph_name, kind)
    m_d, t_d = (v.float().to(dev).requires_grad_(need) for v, need in zip(case[:2], needs))
    cot_d = case[2].float().to(dev)
    poison(dev, (n, C))
    out = ops.softmax_aggregate(m_d, t_d, graph)
    (out * cot_d).sum().backward()
    return out.detach(), [m_d.grad, t_d.grad]


def check_operator(C, graph_name, kind, dev):
    out, grads = run_operator(C, graph_name, kind, dev)
    assert finite(out, *grads), "a row was left unwritten, or an exponential overflowed"
    want = GH.reference(C, graph_name, kind)
    assert grads[1].shape == want[1][1].shape
    assert close(out, want[0], FWD_TOL), "forward"
    for name, got, ref in zip(GH.NAMES[1:], grads, want[1]):
        assert close(got, ref, GRAD_TOL), name
    if graph_name == "no_edges":  # exact zeros, not small numbers
        for v in [out] + grads:
            assert v.abs().max().item() == 0.0
    if graph_name == "random":    # rows without in-edges / sources without out-edges: exact zeros
        assert out[:20].abs().max().item() == 0.0 and grads[0][20:40].abs().max().item() == 0.0
    return out, grads


@pytest.mark.parametrize("kind", GH.ORDER1_KINDS)
@pytest.mark.parametrize("graph", GH.GRAPH_NAMES)
@pytest.mark.parametrize("C", GH.WIDTHS)
def test_aggregate_forward_backward(dev, C, graph, kind):
    """Forward, g_m and g_t at t = 1 and at a temperature per channel from [-2, 4]."""
    from rgb_experiment_amd import ops
    assert ops.softmax_aggregate_supported(C)
    check_operator(C, graph, kind, dev)


@pytest.mark.parametrize("kind", GH.LARGE_KINDS)
@pytest.mark.parametrize("graph", GH.LARGE_GRAPHS)
@pytest.mark.parametrize("C", GH.LARGE_WIDTHS)
def test_aggregate_large_scores(dev, C, graph, kind):
    """t = +-128 (|t m| up to ~600, half of the slots beyond log FLT_MAX: tests/test_genconv_host.py asserts it), at the
    unchanged tolerances."""
    check_operator(C, graph, kind, dev)


def test_aggregate_refusals(dev):
    from rgb_experiment_amd import ops
    _, n = T.graph_of("random")
    graph = operator_graph("random", dev)
    g = torch.Generator().manual_seed(3)
    wide = lambda w: torch.randn(n, w, generator=g).to(dev)
    one = torch.ones(1, device=dev)
    assert not ops.softmax_aggregate_supported(67) and not ops.softmax_aggregate_supported(130)
    with pytest.raises(RuntimeError, match="pad the width"):
        ops.softmax_aggregate(wide(67), one, graph)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.softmax_aggregate(wide(8)[:5], one, graph)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.softmax_aggregate(wide(16), torch.ones(8, device=dev), graph)

    class Partitioned:
        is_distributed = True
    with pytest.raises(RuntimeError, match="no node-partitioned form"):
        ops.softmax_aggregate(wide(8), one, Partitioned())


@pytest.mark.parametrize("kind", GH.ORDER1_KINDS)
@pytest.mark.parametrize("graph", ["random", "powerlaw"])
def test_partial_gradients(dev, graph, kind):
    """m alone, t alone and both: the same bits where a gradient is asked for, None elsewhere."""
    C = 40
    _, full = run_operator(C, graph, kind, dev)
    _, only_m = run_operator(C, graph, kind, dev, needs=(True, False))
    assert only_m[1] is None and torch.equal(only_m[0], full[0])
    _, only_t = run_operator(C, graph, kind, dev, needs=(False, True))
    assert only_t[0] is None and torch.equal(only_t[1], full[1])


def test_partial_gradients_skip_the_record_kernels(dev):
    """Counted at the entry points' timing labels: without a gradient for t the backward runs in its form without g_t
    (no record kept, no reduction launched); without any gradient no backward runs at all."""
    from rgb_experiment_amd import ops
    graph = operator_graph("random", dev)
    case = GH.operator_case(8, "random", "channel")
    for needs, want in (((True, False), [("softmax_aggr_fwd", None), ("softmax_aggr_bwd", None)]),
                        ((False, True), [("softmax_aggr_fwd", None), ("softmax_aggr_bwd", "g_t")]),
                        ((True, True), [("softmax_aggr_fwd", None), ("softmax_aggr_bwd", "g_t")]),
                        ((False, False), [("softmax_aggr_fwd", None)])):
        m, t = (v.float().to(dev).requires_grad_(need) for v, need in zip(case[:2], needs))
        free = torch.ones(1, device=dev, requires_grad=True)   # keeps the node in the autograd graph in the last form
        sink = []
        ops.set_event_sink(sink)
        try:
            (ops.softmax_aggregate(m, t, graph).sum() * free).backward()
        finally:
            ops.set_event_sink(None)
        torch.cuda.synchronize()
        got = [(str(kind), getattr(kind, "variant", None)) for kind, _, _ in sink if str(kind).startswith("softmax_aggr")]
        assert got == want, (needs, got)


@pytest.mark.parametrize("kind", GH.ORDER1_KINDS)
@pytest.mark.parametrize("graph", ["random", "powerlaw"])
def test_inference_form_stores_the_same_bits(dev, graph, kind):
    from rgb_experiment_amd import ops
    g = operator_graph(graph, dev)
    m, t = (v.float().to(dev) for v in GH.operator_case(40, graph, kind)[:2])
    with torch.no_grad():
        plain = ops.softmax_aggregate(m, t, g)
    saved = ops.softmax_aggregate(m.clone().requires_grad_(True), t, g)
    assert saved.grad_fn is not None and plain.grad_fn is None
    assert torch.equal(plain, saved.detach())


def test_two_runs_are_bit_identical(dev):
    """No float atomics and fixed summation orders: forward and backward twice on the hub-row graph, same bits."""
    (out_a, grads_a), (out_b, grads_b) = [run_operator(64, "powerlaw", "channel", dev) for _ in range(2)]
    assert torch.equal(out_a, out_b)
    for a, b in zip(grads_a, grads_b):
        assert torch.equal(a, b)


def test_a_column_block_is_taken_as_it_is(dev):
    """m as a view into a wider matrix gives the bits of a matrix of its own."""
    from rgb_experiment_amd import ops
    C = 64
    graph = operator_graph("random", dev)
    m, t = (v.float().to(dev) for v in GH.operator_case(C, "random", "channel")[:2])
    h = torch.cat([torch.zeros(m.size(0), 8, device=dev), m, torch.zeros(m.size(0), 4, device=dev)], dim=1)
    with torch.no_grad():
        assert torch.equal(ops.softmax_aggregate(m, t, graph), ops.softmax_aggregate(h[:, 8:8 + C], t, graph))


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
@pytest.mark.parametrize("same_width,learn_t,per_channel_t", GH.LAYER_FLAGS)
@pytest.mark.parametrize("C", GH.LAYER_WIDTHS)
def test_layer_forward_backward(dev, C, same_width, learn_t, per_channel_t, train):
    from rgb_experiment_amd.nn import GATConv
    x, ei, ref = GH.layer_case(C, same_width, learn_t, per_channel_t)
    conv = GH.product_layer(ref, x.size(1), C, learn_t=learn_t, per_channel_t=per_channel_t)
    conv.to(dev).train(train)
    ref.train(train)
    assert (GATConv.kernel_channels(C) != C) == (C in (67, 130))
    assert ("t" in dict(conv.named_parameters())) == learn_t
    compare_layer(conv, ref, x, ei, dev)


def test_layer_with_a_deeper_mlp(dev):
    x, ei, ref = GH.layer_case(7, False, True, True, num_layers=3)
    conv = GH.product_layer(ref, x.size(1), 7, learn_t=True, per_channel_t=True, num_layers=3).to(dev).train()
    compare_layer(conv, ref.train(), x, ei, dev)


SWEEP_SEEDS = list(range(24))


def sweep_draw(seed):
    g = torch.Generator().manual_seed(seed)
    draw = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    n = draw(2, 300)
    shape = dict(n=n, E=draw(0, 8 * n), C=draw(1, 140), same_width=bool(draw(0, 1)), f=draw(1, 40),
                 learn_t=bool(draw(0, 1)), per_channel_t=bool(draw(0, 1)), train=bool(draw(0, 1)))
    if shape["same_width"]:
        shape["f"] = shape["C"]
    ei = torch.randint(0, n, (2, shape["E"]), generator=g)
    x = T.f32_exact((n, shape["f"]), g)
    ref = GH.RefGENConv(shape["f"], shape["C"], learn_t=shape["learn_t"], per_channel_t=shape["per_channel_t"])
    GH.set_parameters(ref, g)
    return shape, x, ei, ref.train(shape["train"])


@functools.lru_cache(maxsize=None)
def sweep_case(seed):
    """One draw of the sweep: n in [2, 300], E in [0, 8 n], C in [1, 140], in == out or an input width in [1, 40],
    learn_t, per_channel_t, train; edges uniform over the node pairs (self-loops and duplicates as they fall),
    x ~ N(0, 1), t from [-2, 4], parameters as in tests/test_genconv_host.layer_case. A draw with a ReLU input inside
    the kink margin (tests/test_genconv_host.relu_margin: its gradients are not determined in float32) is drawn again
    from the next sub-seed. -> (shape dict, x, edge_index, reference layer)."""
    for attempt in range(20):
        shape, x, ei, ref = sweep_draw(79000 + seed + 1000 * attempt)
        if GH.relu_margin(lambda: copy.deepcopy(ref)(x, ei)) >= GH.KINK_MARGIN:
            return dict(shape, attempt=attempt), x, ei, ref
    raise AssertionError(f"no well-posed draw for seed {seed}")


@pytest.mark.parametrize("seed", SWEEP_SEEDS)
def test_layer_sweep(dev, seed):
    """The layer forward and backward against the restatement on a drawn shape; the draw is checked for well-posedness
    first (float32 on the CPU, reversed edge order, a quarter of the tolerance)."""
    shape, x, ei, ref = sweep_case(seed)
    ref.zero_grad()
    print(shape)
    assert GH.relu_margin(lambda: copy.deepcopy(ref)(x, ei)) >= GH.KINK_MARGIN
    low = copy.deepcopy(ref).float()
    with torch.no_grad():
        assert T.share_of_tolerance(low(x.float(), ei, reverse=True), copy.deepcopy(ref)(x, ei), FWD_TOL) <= T.WELL_POSED_SHARE
    conv = GH.product_layer(ref, shape["f"], shape["C"], learn_t=shape["learn_t"], per_channel_t=shape["per_channel_t"])
    compare_layer(conv.to(dev).train(shape["train"]), ref, x, ei, dev, cot_seed=seed)


def test_sweep_draws_cover_the_space():
    shapes = [sweep_case(s)[0] for s in SWEEP_SEEDS]
    from rgb_experiment_amd.nn import GATConv
    for flag in ("same_width", "learn_t", "per_channel_t", "train"):
        assert {s[flag] for s in shapes} == {True, False}, flag
    assert any(GATConv.kernel_channels(s["C"]) != s["C"] for s in shapes)          # padded widths
    assert any(s["C"] > 128 for s in shapes) and any(s["C"] <= 16 for s in shapes)
    assert any(s["C"] % 2 == 1 for s in shapes) and any(s["C"] % 4 == 0 for s in shapes)


# ---- model, experiment() ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("train", [False, True])
def test_model_against_restatement(dev, train):
    """Logits, `emb` and every parameter gradient (the temperatures' included): in eval mode, and in training mode
    (BatchNorm on batch statistics) with dropout_rate = 0."""
    x, y, ei, model, ref = GH.model_case()
    model.to(dev).train(train)
    ref.train(train)
    res = model(x.float().to(dev), ei.to(dev))
    want = ref(x, ei)
    assert set(res.keys()) == {"out", "emb", "x"}
    assert close(res["emb"], want["emb"], FWD_TOL) and close(res["out"], want["out"], FWD_TOL)
    torch.nn.functional.nll_loss(res["out"], y.to(dev)).backward()
    torch.nn.functional.nll_loss(want["out"], y).backward()
    refp, got = dict(ref.named_parameters()), dict(model.named_parameters())
    assert sorted(got) == sorted(refp) and "convs.1.t" in got
    for name, prm in got.items():
        assert prm.grad is not None and close(prm.grad, refp[name].grad, GRAD_TOL), name


def test_model_applies_dropout(dev):
    """dropout_rate > 0: the training forward is finite and differs between two steps; the eval forward does not."""
    x, y, ei, model, ref = GH.model_case(dropout_rate=0.5)
    model.to(dev).train()
    xd, eid = x.float().to(dev), ei.to(dev)
    torch.manual_seed(0)
    a, b = model(xd, eid)["emb"].detach(), model(xd, eid)["emb"].detach()
    assert finite(a, b) and not torch.equal(a, b)
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(xd, eid)["emb"], model(xd, eid)["emb"])


def test_experiment_trains_and_hip_graph_equals_eager(dev):
    """Eager against the captured epoch: the same five numbers and the same histories, and the learned temperature has
    moved, by the same amount on both routes (a temperature frozen at capture would stay where the capture found it)."""
    import rgb_experiment_amd as R
    n, f, c, epochs = 300, 16, 4, 5
    gen = torch.Generator().manual_seed(11)
    ei = rand_graph(n, 1800, 13, loops=4, dups=4)
    data = R.Data(x=torch.randn(n, f, generator=gen), y=torch.randint(0, c, (n,), generator=gen), edge_index=ei)
    params = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0, "learn_t": True}
    runs = []
    for graphed in (False, True):
        runs.append(R.experiment(params, specify_data=True, data=data, model_name="deepergcn", learning_rate=0.01,
                                 epoch=epochs, need_to_reappear=True, print_print=False, return_model=True,
                                 use_hip_graph=graphed, implement_early_stopping=False))
    a, b = runs
    assert isinstance(a["model"], DeeperGCN)
    for key in ("ACC", "precision_score", "recall_score", "f1_macro", "f1_micro"):
        assert key in a and np.isfinite(float(a[key])), key
        assert float(a[key]) == float(b[key]), key
    assert b["used_hip_graph"] and not a["used_hip_graph"]
    assert len(a["history"]["train_loss"]) == epochs and len(b["history"]["train_loss"]) == epochs
    for key in ("train_loss", "val_loss", "test_loss"):
        assert np.allclose(a["history"][key], b["history"][key], rtol=0, atol=1e-6), key
    for key in ("train_acc", "val_acc", "test_acc"):
        assert a["history"][key] == b["history"][key], key
    for run in runs:
        for conv in run["model"].convs:
            assert isinstance(conv.t, torch.nn.Parameter) and abs(conv.t.item() - 1.0) > 1e-3   # Adam: ~lr per step
    for ca, cb in zip(a["model"].convs, b["model"].convs):
        assert abs(ca.t.item() - cb.t.item()) < 1e-5
