"""std / var and one-pass multi-aggregation on the MI355X: ops.spmm_multi_raw / propagate_multi / propagate_std /
propagate_var against the float64 restatement of tests/test_multi_aggr_host.py on the device's own CSR, the max / min blocks
and both arg EQUAL to ops.spmm_extremum_raw, offset features (where sum(x^2)/n - (sum(x)/n)^2 in fp32 loses the variance),
constant neighbourhoods (var == 0 and std == 0 exactly), SAGEConv with a list, 'std' / 'var' on both SAGE layers, and a
GraphSAGE2 with four aggregates through experiment() (hipGraph replay equal to the eager loop, the loop against float64).

Bars: the project's layer bars (tests/test_gpu_extremum.py) — forward 1e-4 * max(1, |ref|max), gradients 2e-4 *
max(1, |ref|max), every element compared; on offset features the std / var forward is held to 1e-4 * |ref|max WITHOUT the
floor of 1. Extrema involve no rounding and must be EQUAL. Elements whose float64 variance lies in [0.5e-5, 2e-5] sit on
the kink of std (sqrt(max(var, 1e-5)) masked at the floor): they are left out of the std comparison, their cotangent is 0,
and the tests assert that they are at most 0.1 % of the block."""
import functools
import random

import numpy as np
import pytest
import torch

from test_extremum_host import first_extremal_slot
from test_gpu_extremum import GRAPHS, csr_of, device_graph
from test_gpu_fagcn import assert_same_run, planted_partition
from test_gpu_ggnn import close, rand_graph
from test_multi_aggr_host import FOUR, STATS, RefConv, RefStack, ref_multi, ref_stat, ref_var, std_band

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 1e-4, 2e-4
WIDTHS = (4, 7, 64, 256)  # 7: the zero-padded route
CASES = [(name, d) for name in sorted(GRAPHS) for d in WIDTHS] + [("random", 260)]  # 260: the column-block route
COMBOS = (FOUR,) + tuple((a,) for a in STATS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def features(n, d, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g)
    return 50 + 0.05 * x if kind == "offset" else x


@functools.lru_cache(maxsize=None)
def case(name, d, kind):
    """(graph, n, x, (rowptr, col), band): built once per (graph, width, features), shared by the tests, never changed."""
    ei, n = GRAPHS[name]()
    graph = device_graph(ei, n, torch.device("cuda:0"))
    x = features(n, d, kind, 100 + d)
    csr = csr_of(graph)
    return graph, n, x, csr, std_band(csr[0], csr[1], x)


def cotangent(n, d, names, band, seed):
    """N(0, 1) cotangent [n, k*d]; 0 on the std block's elements around the kink."""
    cot = torch.randn(n, len(names) * d, generator=torch.Generator().manual_seed(seed))
    if "std" in names:
        s = names.index("std")
        cot[:, s * d:(s + 1) * d][band] = 0
    return cot


def run_multi(x, graph, names, cot, dev):
    from rgb_experiment_amd import ops
    xd = x.to(dev).requires_grad_(True)
    if names == ("std",) or names == ("var",):  # the single-statistic entry points of the same kernels
        out = (ops.propagate_std if names == ("std",) else ops.propagate_var)(xd, graph)
    else:
        out = ops.propagate_multi(xd, graph, names)
    (out * cot.to(dev)).sum().backward()
    return out.detach(), xd.grad


def few(band):
    print(f"{int(band.sum())} of {band.numel()} elements around the kink of std")
    return band.sum().item() <= 1e-3 * band.numel()


def check_forward(out, ref, names, d, band, tol=FWD_TOL, floor=1.0):
    """Every block of out [n, k*d] against ref (float64); std without the elements around its kink."""
    got = out.cpu().double()
    for s, a in enumerate(names):
        g, r = got[:, s * d:(s + 1) * d], ref[:, s * d:(s + 1) * d].detach()
        if a in ("max", "min"):
            assert torch.equal(g, r), a
            continue
        keep = ~band if a == "std" else torch.ones_like(band)
        err, scale = ((g - r).abs() * keep).max().item(), max(floor, r.abs().max().item())
        print(f"{a}: max |diff| {err:.3e}, bar {tol * scale:.3e}")
        assert err < tol * scale, a


@pytest.mark.parametrize("name,d", CASES)
def test_forward_all_statistics_from_one_pass(dev, name, d):
    from rgb_experiment_amd import ops
    graph, n, x, (rowptr, col), band = case(name, d, "normal")
    if name == "powerlaw":
        assert graph.fwd.split is not None and graph.bwd.split is not None  # the row split runs on both sides
    assert few(band)
    x64 = x.double()
    ref = ref_multi(rowptr, col, x64, STATS)
    xd = x.to(dev)
    out, amax, amin, kept = ops.spmm_multi_raw(graph.fwd, xd, STATS, True)
    assert out.shape == (n, 6 * d) and kept == {} and amax.dtype == torch.int32 and amin.dtype == torch.int32
    check_forward(out, ref, STATS, d, band)
    # the extrema are the extremum kernel's, value for value and slot for slot, and the restatement's
    xp = torch.nn.functional.pad(xd, (0, (-d) % 4))
    for mode, arg, s in (("max", amax, 4), ("min", amin, 5)):
        raw, raw_arg = ops.spmm_extremum_raw(graph.fwd, xp, mode, True)
        assert torch.equal(out[:, s * d:(s + 1) * d], raw[:, :d]) and torch.equal(arg, raw_arg[:, :d])
        assert torch.equal(arg.cpu().long(), first_extremal_slot(rowptr, col, x64, mode))
    # the inference form: the same bits, no arg
    out2, none_a, none_b, _ = ops.spmm_multi_raw(graph.fwd, xd, STATS, False)
    assert none_a is None and none_b is None and torch.equal(out2, out)
    # a list in another order writes the same bits into other blocks; a kept statistic equals its block
    out4, _, _, kept = ops.spmm_multi_raw(graph.fwd, xd, FOUR, False, keep=("var", "mean"))
    for s, a in enumerate(FOUR):
        assert torch.equal(out4[:, s * d:(s + 1) * d], out[:, STATS.index(a) * d:(STATS.index(a) + 1) * d]), a
    assert sorted(kept) == ["var"] and torch.equal(kept["var"], out[:, 2 * d:3 * d])
    with torch.no_grad():
        assert torch.equal(ops.propagate_multi(xd, graph, list(FOUR)), out4)
        assert torch.equal(ops.propagate_std(xd, graph), out[:, 3 * d:4 * d])
        assert torch.equal(ops.propagate_var(xd, graph), out[:, 2 * d:3 * d])


@pytest.mark.parametrize("name,d", CASES)
def test_backward_matches_float64_autograd_and_repeats(dev, name, d):
    graph, n, x, (rowptr, col), band = case(name, d, "normal")
    x64 = x.double().requires_grad_(True)
    ref = {a: ref_stat(rowptr, col, x64, a) for a in STATS}
    for k, names in enumerate(COMBOS):
        cot = cotangent(n, d, names, band, 7 * d + k)
        want = torch.cat([ref[a] for a in names], dim=1)
        (gref,) = torch.autograd.grad((want * cot.double()).sum(), x64, retain_graph=True)
        out, gx = run_multi(x, graph, names, cot, dev)
        assert out.shape == (n, len(names) * d)
        check_forward(out, want, names, d, band)
        assert gx.shape == (n, d) and close(gx, gref, GRAD_TOL), names
        if names in (FOUR, ("std",), ("max",)):
            out_b, gx_b = run_multi(x, graph, names, cot, dev)
            assert torch.equal(out_b, out) and torch.equal(gx_b, gx), names  # fixed order: the same bits in every run


def test_extras_are_kept_only_when_a_gradient_is_wanted(dev, monkeypatch):
    from rgb_experiment_amd import ops
    graph, n, x, _, _ = case("random", 64, "normal")
    asked = []
    real = ops.spmm_multi_raw
    monkeypatch.setattr(ops, "spmm_multi_raw", lambda csr, x, which, want_arg, keep=(), **k: (
        asked.append((want_arg, tuple(keep))), real(csr, x, which, want_arg, keep=keep, **k))[1])
    xd = x.to(dev)
    a = ops.propagate_multi(xd, graph, ["max", "std"])                               # x takes no gradient
    with torch.no_grad():
        b = ops.propagate_multi(xd.clone().requires_grad_(True), graph, ["max", "std"])  # no_grad
    c = ops.propagate_multi(xd.clone().requires_grad_(True), graph, ["max", "std"])
    e = ops.propagate_multi(xd.clone().requires_grad_(True), graph, ["mean", "std"])
    assert asked == [(False, ()), (False, ()), (True, ("mean",)), (True, ())]
    assert not a.requires_grad and not b.requires_grad and c.requires_grad and e.requires_grad
    assert torch.equal(a, b) and torch.equal(a, c.detach())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.propagate_multi(x, graph, ["max", "std"])


@pytest.mark.parametrize("name", ["random", "powerlaw"])
def test_offset_features_keep_their_variance(dev, name):
    """x = 50 + 0.05 randn: neighbourhood variances of about 0.0025 on values of about 50. std and var are held to
    1e-4 * |ref|max with no floor of 1 (an fp32 sum(x^2)/n - (sum(x)/n)^2 is off by the size of the values themselves,
    tests/test_multi_aggr_host.py::test_offset_features_need_the_shifted_second_moment)."""
    d = 64
    graph, n, x, (rowptr, col), band = case(name, d, "offset")
    assert few(band)
    x64 = x.double().requires_grad_(True)
    ref = {a: ref_stat(rowptr, col, x64, a) for a in STATS}
    for k, names in enumerate((("std",), ("var",), FOUR)):
        cot = cotangent(n, d, names, band, 900 + k)
        want = torch.cat([ref[a] for a in names], dim=1)
        (gref,) = torch.autograd.grad((want * cot.double()).sum(), x64, retain_graph=True)
        out, gx = run_multi(x, graph, names, cot, dev)
        if len(names) == 1:
            check_forward(out, want, names, d, band, floor=0.0)  # no floor of 1
        else:
            check_forward(out, want, names, d, band)
            s = names.index("std")
            check_forward(out[:, s * d:(s + 1) * d], ref["std"], ("std",), d, band, floor=0.0)
        err = (gx.cpu().double() - gref).abs().max().item()
        print(f"{names}: gradient max |diff| {err:.3e}, bar {GRAD_TOL * max(1.0, gref.abs().max().item()):.3e}")
        assert close(gx, gref, GRAD_TOL), names


def test_constant_neighbourhoods_have_exactly_zero_variance(dev):
    """Bag-of-words features from {0, 1} (density 0.3) on a graph of mean in-degree 8 with duplicate edges and self-loops
    (tests/test_gpu_extremum.py's tie test): every (row, column) whose gathered values are all equal — degree-1 rows,
    duplicate edges, all-zero columns — has var == 0 and std == 0 exactly; the rest meets the float64 bars."""
    from rgb_experiment_amd import ops
    n, d = 500, 64
    ei = rand_graph(n, 8 * n - 340, 17, loops=40, dups=300)
    graph = device_graph(ei, n, dev)
    x = (torch.rand(n, d, generator=torch.Generator().manual_seed(18)) < 0.3).float()
    rowptr, col = csr_of(graph)
    hi = torch.cat([ref_stat(rowptr, col, x.double(), "max"), ref_stat(rowptr, col, x.double(), "min")], dim=1)
    constant = hi[:, :d] == hi[:, d:]  # max == min (rows without slots: 0 == 0)
    deg = rowptr[1:] - rowptr[:-1]
    assert int((constant & (deg > 1)[:, None]).sum()) > 1000 and int((~constant).sum()) > 1000
    for xs in (x, 3.0 + 0.1 * x):  # 0.1 and 3.1 are no fp32 numbers: still exactly 0
        out, _, _, _ = ops.spmm_multi_raw(graph.fwd, xs.to(dev), ("var", "std", "mean"), False)
        var, std = out[:, :d].cpu(), out[:, d:2 * d].cpu()
        assert (var[constant] == 0).all() and (std[constant] == 0).all()
        band = std_band(rowptr, col, xs)
        check_forward(out, ref_multi(rowptr, col, xs.double(), ("var", "std", "mean")), ("var", "std", "mean"), d, band)


# ---- layers ------------------------------------------------------------------------------------------------------------

LAYER_CASES = [("sage", list(FOUR)), ("sage", ["sum", "var"]), ("sage", ["mean"]), ("sage", "std"), ("sage", "var"),
               ("my", "std"), ("my", "var"), ("my_no_loops", "std"), ("my_no_loops", "var")]


@pytest.mark.parametrize("kind,aggr", LAYER_CASES, ids=lambda v: "+".join(v) if isinstance(v, list) else v)
@pytest.mark.parametrize("cin,cout", [(12, 7), (16, 40)])
def test_layers_against_the_float64_twin(dev, kind, aggr, cin, cout):
    from rgb_experiment_amd.graph import LOOPS_KEEP, LOOPS_REMOVE_ADD
    from rgb_experiment_amd.nn import MySAGEConv, SAGEConv
    n = 300
    ei = rand_graph(n, 2400, 31, loops=25, dups=60)
    my = kind != "sage"
    torch.manual_seed(7)
    conv = MySAGEConv(cin, cout, add_self_loops=kind == "my", aggr=aggr) if my else SAGEConv(cin, cout, aggr=aggr)
    ref = RefConv(cin, cout, aggr, my)
    ref.load_state_dict({k: v.double() for k, v in conv.state_dict().items()}, strict=True)
    g = torch.Generator().manual_seed(34)  # (a seed for which the precondition below holds in every case)
    x = torch.randn(n, cin, generator=g)
    cot = torch.randn(n, cout, generator=g)
    csr = csr_of(device_graph(ei, n, dev, LOOPS_REMOVE_ADD if kind == "my" else LOOPS_KEEP))
    x64 = x.double().requires_grad_(True)
    # precondition: nothing this layer aggregates sits on the kink of std (a rounding there is worth sqrt(1e-5))
    agg_in = ref.lin_l(x64).detach() if my else x64.detach()
    assert int(std_band(csr[0], csr[1], agg_in).sum()) == 0
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


# ---- experiment() ------------------------------------------------------------------------------------------------------

def test_experiment_with_four_aggregates_against_a_float64_loop_and_graph_equals_eager(dev):
    import rgb_experiment_amd as R
    from rgb_experiment_amd.graph import LOOPS_KEEP
    from rgb_experiment_amd.itexperiments import _as_bool_mask, _make_masks
    from rgb_experiment_amd.models import GraphSAGE2
    n, f, c, epochs, lr, seed = 400, 16, 4, 30, 0.01, 14530529
    data = planted_partition(n, c, f, 5)
    init = {"num_layers": 2, "hidden_unit": 32, "dropout_rate": 0.5, "aggr": list(FOUR)}
    kw = dict(specify_data=True, data=data, model_name="graphsage2", learning_rate=lr, epoch=epochs, need_to_reappear=True,
              reappear_seed=seed, print_print=False, return_model=True, implement_early_stopping=False,
              need_all_metrics=False)
    eager = R.experiment(dict(init), use_hip_graph=False, **kw)
    graphed = R.experiment(dict(init), use_hip_graph=True, **kw)
    assert graphed["used_hip_graph"] and not eager["used_hip_graph"]
    assert isinstance(eager["model"], GraphSAGE2) and [cv.aggr for cv in eager["model"].convs] == [FOUR, FOUR]
    assert len(eager["history"]["train_loss"]) == epochs
    assert_same_run(eager, graphed)
    # the same 30 epochs in float64 over the restatement, from the initial state experiment() seeds (reference :305-310)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    start = GraphSAGE2(input_dim=f, output_dim=c, **init)
    ref = RefStack(2, 32, f, c, FOUR, False)
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v.clone() for k, v in start.state_dict().items()},
                        strict=True)
    tm = _as_bool_mask(_make_masks(data.y, "ratio", "6-2-2", 20, 500, 1000, 123456789)[0], n, torch.device("cpu"))
    csr = csr_of(device_graph(data.edge_index, n, dev, LOOPS_KEEP))
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
