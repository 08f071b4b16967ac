"""PNAConv on the MI355X: ops.pna_aggregate (every lane-group count of the layout, towers, width 320 through the column
blocks, hub rows in both CSRs, rows of exactly 0 / 1 / 64 / 65 / T / T + 1 slots, rows without in-edges, sources without
out-edges, graphs of one to three nodes, a graph without edges, planted ties and constant neighbourhoods, every aggregator
and scaler), selective backward passes, strided and offset operands, PNAConv, the PNA model and
experiment(model_name="pna") against the float64 restatement of tests/test_pna_host.py. The cases are that file's; it
checks on the CPU that each is well-posed.

Tolerances are the project's for this depth of fp32 gather (tests/test_gpu_transformer.py): forward
1e-4 * max(1, |ref|max), gradients 2e-4 * max(1, |ref|max). Every element is compared.

Rows the kernels have no slot for. The op allocates its output and its gradients with torch.empty. Before every operator
call the allocator's free blocks of those sizes are filled with NaN (`poison`), so a row or a slot that a kernel skipped
shows as NaN in the comparison instead of passing on stale zeros; `finite` is asserted on top."""
import functools

import numpy as np
import pytest
import torch

import test_gine_host as G
import test_pna_host as P
import test_transformer_host as T
from test_gpu_ggnn import close
from test_gpu_transformer import device_graph, finite, poison
from test_pna_host import PNA, PNAConv

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = T.FWD_TOL, T.GRAD_TOL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def operator_graph(name, dev):
    """The device graph of a host-file graph, with what the cases rely on asserted once."""
    ei, n = P.graph_of(name)
    graph = device_graph(ei, n, dev)
    assert graph.fwd.nnz == ei.size(1) and graph.bwd.nnz == ei.size(1)        # nothing added, nothing coalesced
    if ei.size(1):   # slot p of the device's CSR is edge order[p] of the host file
        assert torch.equal(graph.fwd.perm[:graph.fwd.nnz].cpu().long(), P.slots_of(name)[3])
    if name == "powerlaw":
        assert graph.fwd.split is not None and graph.bwd.split is not None    # both split plans are in use
    if name == "degrees":
        assert graph.fwd.split["n_long"] == 1 and graph.bwd.split["n_long"] == 1
    return graph


def run_operator(case, graph_name, dev, aggregators, scalers, F, with_a=True, needs=(True, True, True), sink=None,
                 avg=None):
    """ops.pna_aggregate forward and the gradients asked for (`needs`: of a, b, c_slot); -> (out, [g_a, g_b, g_c]), g_c
    in forward CSR slot order."""
    from rgb_experiment_amd import ops
    ei, n = P.graph_of(graph_name)
    graph = operator_graph(graph_name, dev)
    order = P.slots_of(graph_name)[3]
    a, b, c = case
    a = a.float().to(dev).requires_grad_(needs[0]) if with_a else None
    b = b.float().to(dev).requires_grad_(needs[1])
    c = None if c is None else c[order].float().to(dev).requires_grad_(needs[2])
    avg = (P.avg_of(graph_name) if avg is None else avg).to(dev)
    d = b.size(1)
    wide = (d // F) * len(scalers) * len(aggregators) * F
    poison(dev, (n, d), (n, wide), (max(ei.size(1), 1), d))
    if sink is not None:
        ops.set_event_sink(sink)
    try:
        out = ops.pna_aggregate(a, b, c, graph, aggregators, scalers, avg, F)
        cot = P.cotangent(n, wide, 99).float().to(dev)
        if any(t is not None and t.requires_grad for t in (a, b, c)):
            (out * cot).sum().backward()
    finally:
        ops.set_event_sink(None)
    return out.detach(), [None if t is None else t.grad for t in (a, b, c)]


def check(got, want, graph_name):
    out, grads = got
    ref_out, ref_grads, info = want
    order = P.slots_of(graph_name)[3]
    assert out.shape == ref_out.shape and finite(out), "a row was left unwritten"
    err = (out.cpu().double() - ref_out).abs().max().item()
    print(f"forward max |diff| {err:.3e} of max |ref| {ref_out.abs().max().item():.3e}")
    assert close(out, ref_out, FWD_TOL), "forward"
    for name, g, r in zip(("g_a", "g_b", "g_c"), grads, ref_grads):
        if r is None:   # absent, or (var / std alone) without any influence: no gradient, or exact zeros
            assert g is None or g.abs().max().item() == 0.0, name
            continue
        assert g is not None and finite(g), name + ": a row or a slot was left unwritten"
        r = r[order] if name == "g_c" else r
        assert g.shape == r.shape, name
        if r.numel():
            print(f"{name} max |diff| {(g.cpu().double() - r).abs().max().item():.3e} of max |ref| {r.abs().max().item():.3e}")
            assert close(g, r, GRAD_TOL), name
    empty = (info["deg"] == 0).nonzero(as_tuple=True)[0].to(out.device)
    assert out[empty].abs().max().item() == 0.0 if empty.numel() else True     # rows without slots: exact zeros


@pytest.mark.parametrize("d,F,graph", P.OPERATOR_CASES)
def test_aggregate_forward_backward(dev, d, F, graph):
    from rgb_experiment_amd import ops
    assert ops.pna_supported(min(d, 256), F)
    got = run_operator(P.operator_case(d, graph), graph, dev, P.DEFAULT_AGGR, P.DEFAULT_SCALERS, F)
    check(got, P.reference(d, F, graph), graph)


OPTIONS = ([((k,), P.DEFAULT_SCALERS) for k in P.AGGREGATORS] + [(P.DEFAULT_AGGR, (s,)) for s in P.SCALERS]
           + [(P.AGGREGATORS, P.SCALERS), (("std", "min", "sum"), ("linear", "identity"))])


@pytest.mark.parametrize("aggregators,scalers", OPTIONS, ids=lambda v: "+".join(v))
@pytest.mark.parametrize("with_a,with_c", [(True, True), (True, False), (False, True), (False, False)])
def test_option_space(dev, aggregators, scalers, with_a, with_c):
    """Every aggregator and every scaler alone, all 6 x 5, an order that is not the bit order; a and c present or absent."""
    d, graph = P.OPTION_CASE
    case = P.operator_case(d, graph, with_c)
    got = run_operator(case, graph, dev, aggregators, scalers, d, with_a=with_a)
    check(got, P.run_formula(case, graph, aggregators, scalers, d, with_a=with_a), graph)


def test_all_options_on_the_hub_graph(dev):
    case = P.operator_case(32, "powerlaw")
    got = run_operator(case, "powerlaw", dev, P.AGGREGATORS, P.SCALERS, 16)
    check(got, P.run_formula(case, "powerlaw", P.AGGREGATORS, P.SCALERS, 16), "powerlaw")


def test_two_runs_are_bit_identical(dev):
    case = P.operator_case(64, "powerlaw")
    (out_a, grads_a), (out_b, grads_b) = [run_operator(case, "powerlaw", dev, P.AGGREGATORS, P.SCALERS, 16)
                                          for _ in range(2)]
    assert torch.equal(out_a, out_b)
    for a, b in zip(grads_a, grads_b):
        assert torch.equal(a, b)


@pytest.mark.parametrize("graph", ["random", "powerlaw"])
def test_planted_ties_and_constant_neighbourhoods_are_exact(dev, graph):
    """Duplicate edges with identical c rows: the lowest slot takes the whole extremum gradient, the other exactly 0. A
    neighbourhood of equal u: var == 0 and std == 0 EXACTLY, and every slot's g_c from them is exactly 0."""
    d = 32
    case = P.operator_case(d, graph)
    ei, n = P.graph_of(graph)
    order = P.slots_of(graph)[3]
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.numel())
    pairs, const = P.planted(graph)
    out, grads = run_operator(case, graph, dev, ("max", "min"), ("identity",), d, with_a=False)
    cot = P.cotangent(n, 2 * d, 99).float()
    for p, q in pairs:
        lo, hi = sorted((int(inv[p]), int(inv[q])))
        r = int(ei[1, p])
        assert grads[2][lo, 0].item() == cot[r, 0].item() and grads[2][hi, 0].item() == 0.0          # the max of channel 0
        assert grads[2][lo, 1].item() == cot[r, d + 1].item() and grads[2][hi, 1].item() == 0.0      # the min of channel 1
    out, grads = run_operator(case, graph, dev, ("var", "std", "mean"), ("identity", "amplification"), d)
    assert out[const, :2 * d].abs().max().item() == 0.0 and out[const, 3 * d:5 * d].abs().max().item() == 0.0
    assert torch.allclose(out[const, 2 * d:3 * d].cpu(), 3.0 + case[0][const].float(), rtol=1e-6, atol=0)   # mean = 3 + a
    out, grads = run_operator(case, graph, dev, ("std",), ("identity",), d)
    slots = inv[(ei[1] == const).nonzero(as_tuple=True)[0]].to(dev)
    assert grads[2][slots].abs().max().item() == 0.0                                                  # std == 0: no gradient


def test_offset_keeps_the_variance(dev):
    """b + 1000: var and std against the float64 restatement at the forward tolerance of THEIR OWN scale."""
    d, graph = P.OPTION_CASE
    case = P.operator_case(d, graph, False, 1000.0)
    got = run_operator(case, graph, dev, ("var", "std"), ("identity",), d)
    want = P.run_formula(case, graph, ("var", "std"), ("identity",), d)
    assert want[0].abs().max().item() < 100.0              # the tolerance is on the scale of the spread, not of the offset
    check(got, want, graph)


def test_args_and_identity_blocks_equal_the_multi_aggregation(dev):
    """Without a, c and scalers the kernel computes rgbx_spmm_csr_multi_f32's statistics of b: argmax / argmin equal,
    every identity block bit-equal."""
    from rgb_experiment_amd import ops
    for graph_name, d, F in (("random", 64, 64), ("powerlaw", 64, 16), ("degrees", 32, 32)):
        graph = operator_graph(graph_name, dev)
        b = P.operator_case(d, graph_name)[1].float().to(dev)
        avg = P.avg_of(graph_name).to(dev)
        ref, amax, amin, _ = ops.spmm_multi_raw(graph.fwd, b, P.AGGREGATORS, True)
        out, kept = ops.pna_fwd_raw(graph.fwd, None, b, None, avg, P.AGGREGATORS, ("identity", "linear"), F,
                                    keep=("mean", "std", "argmax", "argmin"))
        assert torch.equal(kept["argmax"], amax) and torch.equal(kept["argmin"], amin)
        Tn, A = d // F, len(P.AGGREGATORS)
        blocks = out.view(-1, Tn, 2, A, F)[:, :, 0]                                 # [N, T, A, F]: the identity scaler
        assert torch.equal(blocks.permute(0, 2, 1, 3).reshape(-1, A * d), ref)
        assert torch.equal(kept["mean"], ref[:, d:2 * d]) and torch.equal(kept["std"], ref[:, 3 * d:4 * d])


@pytest.mark.parametrize("graph", ["random", "powerlaw"])
def test_selective_passes(dev, graph):
    """Only b asks for a gradient: only pna_bwd_src is launched, with the bits of the full backward; only c: only
    pna_bwd_edge; a alone: neither."""
    d = 32
    case = P.operator_case(d, graph)
    args = (P.DEFAULT_AGGR, P.DEFAULT_SCALERS, d)
    _, full = run_operator(case, graph, dev, *args)
    for needs, launched in (((False, True, False), ["pna_fwd", "pna_bwd_src"]),
                            ((False, False, True), ["pna_fwd", "pna_bwd_edge"]),
                            ((True, False, False), ["pna_fwd"]),
                            ((True, True, True), ["pna_fwd", "pna_bwd_edge", "pna_bwd_src"]),
                            ((False, False, False), ["pna_fwd"])):
        sink = []
        _, got = run_operator(case, graph, dev, *args, needs=needs, sink=sink)
        torch.cuda.synchronize()
        assert [str(kind) for kind, _, _ in sink if str(kind).startswith("pna")] == launched
        for need, a, b in zip(needs, got, full):
            assert (a is None) == (not need) and (a is None or torch.equal(a, b))


def test_strided_and_offset_operands(dev):
    """a, b, c as column blocks of wider matrices and a non-contiguous cotangent give the bits of contiguous operands; a c
    view off the 16-byte grid is copied once and gives them too."""
    from rgb_experiment_amd import ops
    d, graph_name = 64, "random"
    graph = operator_graph(graph_name, dev)
    order = P.slots_of(graph_name)[3]
    a, b, c = P.operator_case(d, graph_name)
    a, b, c = a.float().to(dev), b.float().to(dev), c[order].float().to(dev)
    avg = P.avg_of(graph_name).to(dev)
    n = a.size(0)
    cot = P.cotangent(n, 12 * d, 99).float().to(dev)
    pad = torch.nn.functional.pad

    def run(av, bv, cv, cotv, cut):
        av, bv, cv = (t.detach().requires_grad_(True) for t in (av, bv, cv))
        out = ops.pna_aggregate(cut(av, 8), cut(bv, 4), cut(cv, 12), graph, P.DEFAULT_AGGR, P.DEFAULT_SCALERS, avg, 16)
        (out * cotv).sum().backward()
        return out.detach(), [cut(av.grad, 8), cut(bv.grad, 4), cut(cv.grad, 12)]

    plain = run(a, b, c, cot, lambda t, k: t)
    wide = run(pad(a, (8, 8)), pad(b, (4, 12)), pad(c, (12, 4)), cot.t().contiguous().t(), lambda t, k: t[:, k:k + d])
    assert torch.equal(plain[0], wide[0]) and all(torch.equal(x, y) for x, y in zip(plain[1], wide[1]))
    flat = torch.zeros(c.numel() + 1, device=dev)
    flat[1:] = c.reshape(-1)
    off_grid = flat[1:].view_as(c)
    assert off_grid.data_ptr() % 16 == 4
    off = run(a, b, off_grid, cot, lambda t, k: t)
    assert torch.equal(plain[0], off[0]) and all(torch.equal(x, y) for x, y in zip(plain[1], off[1]))


def test_aggregate_refusals(dev):
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_REMOVE_ADD, get_graph
    _, n = P.graph_of("random")
    graph = operator_graph("random", dev)
    rows = lambda r, w: torch.zeros(r, w, device=dev)
    avg, nnz = torch.ones(2, device=dev), graph.fwd.nnz
    with pytest.raises(RuntimeError, match="pad the tower width"):
        ops.pna_aggregate(None, rows(n, 12), None, graph, ["mean"], ["identity"], avg, 6)
    with pytest.raises(RuntimeError, match="pad the tower width"):
        ops.pna_aggregate(None, rows(n, 64), None, graph, ["mean"], ["identity"], avg, 24)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.pna_aggregate(None, rows(n, 16), rows(nnz - 1, 16), graph, ["mean"], ["identity"], avg, 16)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.pna_aggregate(rows(n, 8), rows(n, 16), None, graph, ["mean"], ["identity"], avg, 16)
    with pytest.raises(RuntimeError, match="avg_deg"):
        ops.pna_aggregate(None, rows(n, 16), None, graph, ["mean"], ["identity"], torch.ones(3, device=dev), 16)
    with pytest.raises(ValueError):
        ops.pna_aggregate(None, rows(n, 16), None, graph, ["median"], ["identity"], avg, 16)
    with pytest.raises(RuntimeError, match="LOOPS_KEEP"):
        ops.pna_aggregate(None, rows(n, 16), None, get_graph(graph._keepalive, n, LOOPS_REMOVE_ADD), ["mean"],
                          ["identity"], avg, 16)


def test_degree_averages_on_the_device(dev):
    from rgb_experiment_amd import ops
    for name in P.OWN_AVG_GRAPHS:
        got = ops.degree_averages(operator_graph(name, dev))
        assert got.is_cuda and torch.allclose(got.cpu(), P.avg_of(name), rtol=1e-6, atol=0)


# ---- layer ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("from_hist", [False, True])
@pytest.mark.parametrize("config", P.LAYER_CONFIGS)
def test_layer_forward_backward(dev, config, from_hist):
    """Output and the gradients of x, of edge_attr and of every parameter against the restatement; T in {1, 4}, with and
    without edge_dim, divide_input both ways, F_in = 6 padded to 8; deg=None (the graph's own averages) and PyG's
    histogram."""
    x, ei, ea, ref, avg = P.layer_case(config)
    hist = torch.bincount(torch.bincount(ei[1], minlength=P.LAYER_N)) if from_hist else None
    conv = P.product_layer(ref, config, deg=hist).to(dev)
    xd = x.float().to(dev).requires_grad_(True)
    ead = None if ea is None else ea.float().to(dev).requires_grad_(True)
    out = conv(xd, ei.to(dev), ead)
    assert torch.allclose(conv.avg_deg.cpu(), avg, rtol=1e-6, atol=0)
    xr = x.clone().requires_grad_(True)
    ear = None if ea is None else ea.clone().requires_grad_(True)
    want = ref(xr, ei, ear)
    assert out.shape == want.shape and finite(out) and close(out, want, FWD_TOL), "forward"
    cot = T.f32_exact(want.shape, torch.Generator().manual_seed(17))
    (out * cot.float().to(dev)).sum().backward()
    (want * cot).sum().backward()
    assert close(xd.grad, xr.grad, GRAD_TOL), "g_x"
    if ea is not None:
        assert close(ead.grad, ear.grad, GRAD_TOL), "g_edge_attr"
    refp, got = dict(ref.named_parameters()), dict(conv.named_parameters())
    assert sorted(got) == sorted(refp)
    for key, prm in got.items():
        assert prm.grad is not None and finite(prm.grad) and close(prm.grad, refp[key].grad, GRAD_TOL), key


# ---- model, experiment() ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_edges", [False, True])
def test_model_against_restatement(dev, with_edges):
    """Logits, `emb` and every parameter gradient of one training step."""
    x, y, ei, ea, model, ref = P.model_case(with_edges)
    model.to(dev).train()
    ref.train()
    res = model(x.float().to(dev), ei.to(dev), None if ea is None else ea.float().to(dev))
    want = ref(x, ei, ea)
    assert {"out", "emb"} <= set(res.keys())
    assert close(res["emb"], want["emb"], FWD_TOL) and close(res["out"], want["out"], FWD_TOL)
    torch.nn.functional.nll_loss(res["out"], y.to(dev)).backward()
    torch.nn.functional.nll_loss(want["out"], y).backward()
    refp, got = dict(ref.named_parameters()), dict(model.named_parameters())
    assert sorted(got) == sorted(refp)
    for name, prm in got.items():
        assert prm.grad is not None and close(prm.grad, refp[name].grad, GRAD_TOL), name


@pytest.mark.parametrize("with_edges", [False, True])
def test_experiment_trains_and_hip_graph_equals_eager(dev, with_edges):
    """A separable toy: the label is the sign pattern of two feature columns, which the neighbours share."""
    import rgb_experiment_amd as R
    from test_gpu_ggnn import rand_graph
    n, f, c, d, epochs = 300, 8, 4, 5, 6
    gen = torch.Generator().manual_seed(21)
    y = torch.randint(0, c, (n,), generator=gen)
    x = torch.randn(n, f, generator=gen) * 0.3
    x[:, 0] += (y % 2).float() * 2 - 1
    x[:, 1] += (y // 2).float() * 2 - 1
    ei = rand_graph(n, 1500, 23, loops=4, dups=4)
    ei = ei[:, y[ei[0]] == y[ei[1]]].contiguous()                            # edges inside the classes
    data = R.Data(x=x, y=y, edge_index=ei, edge_attr=torch.randn(ei.size(1), d, generator=gen))
    params = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0, "towers": 2}
    if with_edges:
        params["edge_dim"] = d
    runs = []
    for graphed in (False, True):
        runs.append(R.experiment(params, specify_data=True, data=data, model_name="pna", learning_rate=0.01,
                                 epoch=epochs, need_to_reappear=True, print_print=False, return_model=True,
                                 use_hip_graph=graphed, implement_early_stopping=False, use_edge_attr=with_edges))
    a, b = runs
    assert isinstance(a["model"], PNA)
    for key in ("ACC", "precision_score", "recall_score", "f1_macro", "f1_micro"):
        assert key in a and np.isfinite(float(a[key])), key
    assert b["used_hip_graph"] and not a["used_hip_graph"]
    assert len(a["history"]["train_loss"]) == epochs and len(b["history"]["train_loss"]) == epochs
    assert all(np.isfinite(v) for v in a["history"]["train_loss"])
    for key in ("train_loss", "val_loss", "test_loss"):
        assert np.allclose(a["history"][key], b["history"][key], rtol=0, atol=1e-6), key
    for key in ("train_acc", "val_acc", "test_acc"):
        assert a["history"][key] == b["history"][key], key
    sa, sb = a["model"].state_dict(), b["model"].state_dict()               # both loops train bit-identically
    assert sorted(sa) == sorted(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert a["history"]["train_loss"][-1] < a["history"]["train_loss"][0]
    for run in runs:                                                         # the averages came from the graph, on the device
        assert all(conv._avg_known and float(conv.avg_deg[0]) > 0 for conv in run["model"].convs)
