"""max / min / sum neighbourhood aggregation on the MI355X: ops.propagate_max / propagate_min (forward bit-equal to the
float64 restatement of tests/test_extremum_host.py on the device's own CSR, values AND winning slots; backward against
autograd through the restatement's gather, and bit-equal from run to run), bag-of-words features where most extrema are
tied, SAGEConv / MySAGEConv / GraphSAGE / GraphSAGE2 with the `aggr` keyword, experiment() against a float64 loop with
the hipGraph replay equal to the eager loop, and one forward + backward at workload L on sampled rows.

Bars: an extremum involves no rounding, so the op's forward must be EQUAL (values and arg). Gradients and everything
behind a Linear are fp32 sums against float64: forward 1e-4 * max(1, |ref|max), gradients 2e-4 * max(1, |ref|max) — the
project's bars for a layer against a float64 restatement (tests/test_gpu_fagcn.py). Every element is compared.

The tie test's precondition was evaluated on the CPU when it was written (density 0.3, mean in-degree 8, 500 nodes, 64
columns): 75.8 % of the non-empty (row, channel) pairs are tied between distinct sources for max, 97.6 % for min."""
import copy
import random

import numpy as np
import pytest
import torch

from test_extremum_host import RefSAGEConv, RefSAGEStack, first_extremal_slot, host_csr, ref_extremum
from test_gpu_fagcn import assert_same_run, planted_partition, powerlaw_graph
from test_gpu_ggnn import close, rand_graph

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 1e-4, 2e-4
WIDTHS = (4, 7, 64, 128, 256)  # 7: the zero-padded route


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def no_in_edges_graph():
    """400 nodes; the last 60 are never a target (rows without slots), 25 of them never a source either."""
    g = torch.Generator().manual_seed(21)
    return torch.stack([torch.randint(0, 375, (3000,), generator=g), torch.randint(0, 340, (3000,), generator=g)])


GRAPHS = {
    "random": lambda: (rand_graph(700, 6000, 3), 700),
    "powerlaw": lambda: (powerlaw_graph(), 2000),  # top rows of the forward AND the transposed CSR above 1024 slots
    "dups_loops": lambda: (rand_graph(300, 2000, 5, loops=40, dups=500), 300),
    "no_in_edges": lambda: (no_in_edges_graph(), 400),
}


def device_graph(ei, n, dev, loops_mode=None):
    from rgb_experiment_amd.graph import LOOPS_KEEP, get_graph
    return get_graph(ei.to(dev), n, LOOPS_KEEP if loops_mode is None else loops_mode)


def csr_of(graph):
    """The device's forward CSR on the host: (rowptr, col)."""
    f = graph.fwd
    return f.rowptr.cpu().long(), f.col[:f.nnz].cpu().long()


def run_op(x, graph, mode, cot, dev):
    from rgb_experiment_amd import ops
    xd = x.to(dev).requires_grad_(True)
    out = (ops.propagate_max if mode == "max" else ops.propagate_min)(xd, graph)
    (out * cot.to(dev)).sum().backward()
    return out.detach(), xd.grad


@pytest.mark.parametrize("mode", ["max", "min"])
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_op_forward_is_exact_and_backward_matches_and_repeats(dev, name, d, mode):
    from rgb_experiment_amd import ops
    ei, n = GRAPHS[name]()
    graph = device_graph(ei, n, dev)
    if name == "powerlaw":
        assert graph.fwd.split is not None and graph.bwd.split is not None  # the row split runs on both sides
    if name == "no_in_edges":
        assert int((graph.fwd.rowptr[1:] == graph.fwd.rowptr[:-1]).sum()) >= 60
    g = torch.Generator().manual_seed(100 + d)
    x = torch.randn(n, d, generator=g)
    cot = torch.randn(n, d, generator=g)
    rowptr, col = csr_of(graph)
    x64 = x.double().requires_grad_(True)
    want, want_arg = ref_extremum(rowptr, col, x64, mode)
    (want * cot.double()).sum().backward()

    out, gx = run_op(x, graph, mode, cot, dev)
    assert out.shape == (n, d) and torch.equal(out.cpu().double(), want.detach())
    xp = torch.nn.functional.pad(x, (0, (-d) % 4)).to(dev)
    raw, arg = ops.spmm_extremum_raw(graph.fwd, xp, mode, True)
    assert arg.dtype == torch.int32 and torch.equal(arg[:, :d].cpu().long(), want_arg)
    assert torch.equal(raw[:, :d], out)
    raw2, none = ops.spmm_extremum_raw(graph.fwd, xp, mode, False)  # the inference form
    assert none is None and torch.equal(raw2, raw)
    assert close(gx, x64.grad, GRAD_TOL)
    out_b, gx_b = run_op(x, graph, mode, cot, dev)
    assert torch.equal(out_b, out) and torch.equal(gx_b, gx)  # fixed summation order: the same bits in every run


def test_arg_is_kept_only_when_a_gradient_is_wanted(dev, monkeypatch):
    from rgb_experiment_amd import ops
    ei, n = GRAPHS["random"]()
    graph = device_graph(ei, n, dev)
    asked = []
    real = ops.spmm_extremum_raw
    monkeypatch.setattr(ops, "spmm_extremum_raw", lambda csr, x, mode, want_arg, **k: (asked.append(want_arg), real(csr, x, mode, want_arg, **k))[1])
    x = torch.randn(n, 16, device=dev)
    a = ops.propagate_max(x, graph)                                     # x takes no gradient
    with torch.no_grad():
        b = ops.propagate_max(x.clone().requires_grad_(True), graph)    # no_grad
    c = ops.propagate_min(x.clone().requires_grad_(True), graph)
    assert asked == [False, False, True]
    assert not a.requires_grad and not b.requires_grad and c.requires_grad and torch.equal(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.propagate_max(x.cpu(), graph)


@pytest.mark.parametrize("mode", ["max", "min"])
def test_tied_extrema_take_the_lowest_slot(dev, mode):
    """Bag-of-words features from {0, 1} (density 0.3) on a graph of mean in-degree 8 with duplicate edges and self-loops:
    most (row, channel) pairs have several extremal slots from DISTINCT sources; the lowest slot must win, in the forward
    and in where the backward sends the gradient."""
    from rgb_experiment_amd import ops
    n, d = 500, 64
    ei = rand_graph(n, 8 * n - 340, 17, loops=40, dups=300)
    graph = device_graph(ei, n, dev)
    g = torch.Generator().manual_seed(18)
    x = (torch.rand(n, d, generator=g) < 0.3).float()
    cot = torch.randn(n, d, generator=g)
    rowptr, col = csr_of(graph)
    # precondition: at least half of the non-empty (row, channel) pairs hold >= 2 tied extremal slots of distinct sources
    tied = nonempty = 0
    for i in range(n):
        s, e = int(rowptr[i]), int(rowptr[i + 1])
        if e == s:
            continue
        seg = x[col[s:e]]
        best = seg.max(0).values if mode == "max" else seg.min(0).values
        hit = seg == best[None, :]                                           # [deg, d]
        src = torch.nn.functional.one_hot(col[s:e], n).bool()                # [deg, n]
        distinct = (hit.T.float() @ src.float() > 0).sum(1)                  # [d] distinct extremal sources
        tied += int((distinct >= 2).sum())
        nonempty += d
    print(f"{mode}: {tied} of {nonempty} non-empty (row, channel) pairs are tied between distinct sources")
    assert nonempty > 0 and 2 * tied >= nonempty

    x64 = x.double().requires_grad_(True)
    want, want_arg = ref_extremum(rowptr, col, x64, mode)
    (want * cot.double()).sum().backward()
    out, gx = run_op(x, graph, mode, cot, dev)
    _, arg = ops.spmm_extremum_raw(graph.fwd, x.to(dev), mode, True)
    assert torch.equal(out.cpu().double(), want.detach())
    assert torch.equal(arg.cpu().long(), want_arg)
    assert close(gx, x64.grad, GRAD_TOL)
    assert torch.equal(run_op(x, graph, mode, cot, dev)[1], gx)


# ---- layers ------------------------------------------------------------------------------------------------------------

LAYERS = {"sage": (False, None), "my": (True, True), "my_no_loops": (True, False)}


def make_layer(kind, cin, cout, aggr, seed):
    from rgb_experiment_amd.graph import LOOPS_KEEP, LOOPS_REMOVE_ADD
    from rgb_experiment_amd.nn import MySAGEConv, SAGEConv
    my, loops = LAYERS[kind]
    torch.manual_seed(seed)
    extra = {} if aggr is None else {"aggr": aggr}
    conv = MySAGEConv(cin, cout, add_self_loops=loops, **extra) if my else SAGEConv(cin, cout, **extra)
    return conv, (LOOPS_REMOVE_ADD if (my and loops) else LOOPS_KEEP)


@pytest.mark.parametrize("aggr", ["max", "min", "add"])
@pytest.mark.parametrize("kind", sorted(LAYERS))
@pytest.mark.parametrize("cin,cout", [(12, 7), (16, 40)])
def test_layers_against_the_restatement(dev, kind, aggr, cin, cout):
    n = 300
    ei = rand_graph(n, 2400, 31, loops=25, dups=60)
    conv, loops_mode = make_layer(kind, cin, cout, aggr, 7)
    ref = RefSAGEConv(cin, cout, aggr, LAYERS[kind][0])
    ref.load_state_dict({k: v.double() for k, v in conv.state_dict().items()}, strict=True)
    g = torch.Generator().manual_seed(32)
    x = torch.randn(n, cin, generator=g)
    cot = torch.randn(n, cout, generator=g)
    csr = csr_of(device_graph(ei, n, dev, loops_mode))
    x64 = x.double().requires_grad_(True)
    want = ref(x64, csr)
    (want * cot.double()).sum().backward()

    conv.to(dev)
    xd = x.to(dev).requires_grad_(True)
    out = conv(xd, ei.to(dev))
    (out * cot.to(dev)).sum().backward()
    assert out.shape == (n, cout) and close(out, want, FWD_TOL)
    assert close(xd.grad, x64.grad, GRAD_TOL)
    refp = dict(ref.named_parameters())
    for name, prm in conv.named_parameters():
        assert prm.grad is not None and close(prm.grad, refp[name].grad, GRAD_TOL), name
    with torch.no_grad():  # the inference form: same numbers, nothing kept for a backward
        assert torch.equal(conv(x.to(dev), ei.to(dev)), out.detach())


@pytest.mark.parametrize("kind", sorted(LAYERS))
@pytest.mark.parametrize("cin,cout", [(12, 7), (16, 40), (64, 64)])
def test_aggr_mean_is_the_layer_without_the_keyword(dev, kind, cin, cout):
    n = 300
    ei = rand_graph(n, 2400, 31, loops=25, dups=60).to(dev)
    g = torch.Generator().manual_seed(33)
    x = torch.randn(n, cin, generator=g).to(dev)
    cot = torch.randn(n, cout, generator=g).to(dev)
    results = []
    for aggr in (None, "mean"):
        conv, _ = make_layer(kind, cin, cout, aggr, 7)
        conv.to(dev)
        xd = x.clone().requires_grad_(True)
        out = conv(xd, ei)
        (out * cot).sum().backward()
        with torch.no_grad():
            ev = conv.eval()(x, ei)
        results.append([out.detach(), xd.grad, ev] + [p.grad for p in conv.parameters()])
    assert len(results[0]) == len(results[1])
    for a, b in zip(*results):
        assert torch.equal(a, b)


# ---- models ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["graphsage", "graphsage2"])
def test_models_with_max_against_the_restatement(dev, name):
    from rgb_experiment_amd.graph import LOOPS_KEEP, LOOPS_REMOVE_ADD
    from rgb_experiment_amd.models import GraphSAGE, GraphSAGE2
    n, f, hid, c = 400, 24, 32, 5
    ei = rand_graph(n, 3200, 41, loops=20, dups=50)
    g = torch.Generator().manual_seed(42)
    x = torch.randn(n, f, generator=g)
    y = torch.randint(0, c, (n,), generator=g)
    torch.manual_seed(9)
    my = name == "graphsage"
    model = (GraphSAGE if my else GraphSAGE2)(num_layers=3, hidden_unit=hid, input_dim=f, output_dim=c, dropout_rate=0.5,
                                              aggr="max")
    ref = RefSAGEStack(3, hid, f, c, "max", my)
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v.clone() for k, v in model.state_dict().items()},
                        strict=True)
    csr = csr_of(device_graph(ei, n, dev, LOOPS_REMOVE_ADD if my else LOOPS_KEEP))
    model.to(dev).train()
    ref.train()
    res = model(x.to(dev), ei.to(dev))
    want = ref(x.double(), csr)
    assert close(res["emb"], want, FWD_TOL)
    torch.nn.functional.nll_loss(res["out"], y.to(dev)).backward()
    torch.nn.functional.nll_loss(torch.log_softmax(want, 1), y).backward()
    refp = dict(ref.named_parameters())
    for pname, prm in model.named_parameters():
        assert prm.grad is not None and close(prm.grad, refp[pname].grad, GRAD_TOL), pname
    # the loss taken through the stack's own entry point (the route experiment() uses) is the same number
    loss, stats = model.masked_ce(x.to(dev), ei.to(dev), y.to(dev), None)
    assert abs(loss.item() - torch.nn.functional.nll_loss(torch.log_softmax(ref(x.double(), csr), 1), y).item()) < FWD_TOL
    model.eval()
    ref.eval()
    with torch.no_grad():
        assert model._collapsed_operands() is None
        assert close(model(x.to(dev), ei.to(dev))["emb"], ref(x.double(), csr), FWD_TOL)


# ---- experiment() ------------------------------------------------------------------------------------------------------

def test_experiment_with_max_against_a_float64_loop_and_graph_equals_eager(dev):
    import rgb_experiment_amd as R
    from rgb_experiment_amd.graph import LOOPS_REMOVE_ADD
    from rgb_experiment_amd.itexperiments import _as_bool_mask, _make_masks
    from rgb_experiment_amd.models import GraphSAGE
    n, f, c, epochs, lr, seed = 400, 16, 4, 30, 0.01, 14530529
    data = planted_partition(n, c, f, 5)
    init = {"num_layers": 2, "hidden_unit": 32, "dropout_rate": 0.5, "aggr": "max"}
    kw = dict(specify_data=True, data=data, model_name="graphsage", learning_rate=lr, epoch=epochs, need_to_reappear=True,
              reappear_seed=seed, print_print=False, return_model=True, implement_early_stopping=False,
              need_all_metrics=False)
    eager = R.experiment(dict(init), use_hip_graph=False, **kw)
    graphed = R.experiment(dict(init), use_hip_graph=True, **kw)
    assert graphed["used_hip_graph"] and not eager["used_hip_graph"]
    assert isinstance(eager["model"], GraphSAGE) and [cv.aggr for cv in eager["model"].convs] == ["max", "max"]
    assert len(eager["history"]["train_loss"]) == epochs
    assert_same_run(eager, graphed)
    # the same 30 epochs in float64 over the restatement, from the initial state experiment() seeds (reference :305-310)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    start = GraphSAGE(input_dim=f, output_dim=c, **init)
    ref = RefSAGEStack(2, 32, f, c, "max", True)
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v.clone() for k, v in start.state_dict().items()},
                        strict=True)
    tm = _as_bool_mask(_make_masks(data.y, "ratio", "6-2-2", 20, 500, 1000, 123456789)[0], n, torch.device("cpu"))
    csr = csr_of(device_graph(data.edge_index, n, dev, LOOPS_REMOVE_ADD))
    opt = torch.optim.Adam(ref.parameters(), lr=lr)
    x64, want = data.x.double(), []
    for _ in range(epochs):
        ref.train()
        opt.zero_grad()
        loss = torch.nn.functional.nll_loss(torch.log_softmax(ref(x64, csr), 1)[tm], data.y[tm])
        want.append(loss.item())
        loss.backward()
        opt.step()
    got = eager["history"]["train_loss"]
    worst = max(abs(a - b) for a, b in zip(got, want))
    print(f"loss history: first {got[0]:.6f} / {want[0]:.6f}, last {got[-1]:.6f} / {want[-1]:.6f}, max |diff| {worst:.3e}")
    assert worst < FWD_TOL * max(1.0, max(abs(v) for v in want))
    assert got[-1] < 0.7 * got[0]  # it trains


# ---- workload L --------------------------------------------------------------------------------------------------------

@pytest.mark.slow
def test_max_at_workload_l_on_sampled_rows(dev):
    """|V| = 2 M, |E| = 60 M (bench.py's workload L graph), d = 64, one forward + backward of ops.propagate_max: out and
    g_x of 64 sampled rows. A row's output depends on its in-edges; its input gradient on its out-edges AND on every
    in-edge of the targets they reach (which slot won there). The restatement runs over exactly those edges, kept in
    input order, so its slots are the device's slots in the same order."""
    import bench
    from rgb_experiment_amd import ops
    wl = bench.WORKLOADS["L"]
    N, d = wl["N"], 64
    ei, x, _ = bench.synth(N, wl["E"], d)
    cot = torch.randn(N, d, generator=torch.Generator().manual_seed(4))
    eid = ei.to(dev)
    graph = device_graph(ei, N, dev)
    xd = x.to(dev).requires_grad_(True)
    out = ops.propagate_max(xd, graph)
    (out * cot.to(dev)).sum().backward()
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(9))[:64].to(dev)
    src, dst = eid[0], eid[1]
    is_row = torch.zeros(N, dtype=torch.bool, device=dev)
    is_row[rows] = True
    is_tgt = is_row.clone()
    is_tgt[dst[is_row[src]]] = True        # the sampled rows and every target they feed
    keep = is_tgt[dst]                      # all in-edges of those targets, in input order
    nodes = torch.unique(torch.cat([rows, src[keep], dst[keep]]))
    local = torch.full((N,), -1, dtype=torch.long, device=dev)
    local[nodes] = torch.arange(nodes.numel(), device=dev)
    sub = torch.stack([local[src[keep]], local[dst[keep]]]).cpu()
    nc = nodes.cpu()
    rowptr, col = host_csr(sub, nc.numel())
    xs = x[nc].double().requires_grad_(True)
    want, _ = ref_extremum(rowptr, col, xs, "max")  # (only those targets have slots in the sub-graph)
    (want * cot[nc].double()).sum().backward()
    lr = local[rows].cpu()
    assert torch.equal(out[rows].detach().cpu().double(), want[lr].detach())
    assert close(xd.grad[rows], xs.grad[lr], GRAD_TOL)
