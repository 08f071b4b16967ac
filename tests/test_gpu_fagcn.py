"""FAGCN on the MI355X: FAConv (eval and training mode, fused and composed kernels, hub rows, a graph of self-loops
only), the whole model and experiment(model=FAGCN(...)) against the float64 restatement of tests/test_fagcn_host.py,
which is fed the exact dropout decisions the device made (ops.faconv_random_choices), and one layer forward +
backward at workload L's size on sampled rows.

Tolerances are those tests/test_gpu_supergat.py uses for the same kinds of check (an fp32 gather of the same depth):
forward 1e-4 * max(1, |ref|max), gradients 2e-4 * max(1, |ref|max), model logits 1e-4 and parameter gradients 2e-4,
workload L 1e-4 (forward) / 2e-4 (gradient). Every element is compared."""
import copy

import numpy as np
import pytest
import torch

from test_fagcn_host import RefFAConv, RefFAGCN
from test_gpu_ggnn import close, rand_graph

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 1e-4, 2e-4
FUSED_WIDTHS = (4, 7, 8, 16, 40, 64, 128)
REFUSED_WIDTH = 67  # odd and > 64: more than 64 lanes per row at one float per lane


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def powerlaw_graph():
    """2,000 nodes, 80,000 edges with Zipf-like sources AND targets (bench.powerlaw_endpoints): the top rows of both the
    forward and the transposed CSR exceed graph.LONG_ROW_SLOTS = 1024 and take the chunk + combine kernels."""
    import bench
    return torch.stack([bench.powerlaw_endpoints(2000, 80000, 71), bench.powerlaw_endpoints(2000, 80000, 72)])


GRAPHS = {
    "random": lambda: (rand_graph(700, 6000, 3, loops=11, dups=40), 700),
    "powerlaw": lambda: (powerlaw_graph(), 2000),
    "empty": lambda: (torch.zeros((2, 0), dtype=torch.int64), 50),
}


def make_case(C, n, seed, eps=0.3, p=0.0):
    """(x, x0 float64 [n, C], reference layer): attention vectors N(0, 1/C), so al + ar is of order 1 and tanh works
    on its curved part."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g, dtype=torch.float64)
    x0 = torch.randn(n, C, generator=g, dtype=torch.float64)
    ref = RefFAConv(C, eps=eps, dropout=p)
    with torch.no_grad():
        ref.att_l.weight.copy_(torch.randn(1, C, generator=g, dtype=torch.float64) / C ** 0.5)
        ref.att_r.weight.copy_(torch.randn(1, C, generator=g, dtype=torch.float64) / C ** 0.5)
    return x, x0, ref


def device_layer(ref, C, dev, form, p=0.0):
    from rgb_experiment_amd.nn import FAConv
    conv = FAConv(C, eps=ref.eps, dropout=p)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    conv.form = form
    return conv.to(dev)


def choices_of(conv, ei_dev, n):
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, get_graph
    graph = get_graph(ei_dev, n, LOOPS_ADD_REMAINING)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in ops.faconv_random_choices(conv.last_draw, graph).items()}


def run_layer(C, ei, n, form, dev, train, seed=100, torch_seed=5, eps=0.3):
    """Forward and all four gradients of one layer against the restatement; returns the device output."""
    p = 0.5 if train else 0.0
    x, x0, ref = make_case(C, n, seed, eps=eps, p=p)
    conv = device_layer(ref, C, dev, form, p=p)
    conv.train(train)
    ref.train(train)
    xd = x.float().to(dev).requires_grad_(True)
    x0d = x0.float().to(dev).requires_grad_(True)
    eid = ei.to(dev)
    torch.manual_seed(torch_seed)
    out = conv(xd, x0d, eid)
    ch = choices_of(conv, eid, n) if train else None
    xr, x0r = x.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    want = ref(xr, x0r, ei, ch)
    assert close(out, want, FWD_TOL), "forward"
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64)
    (out * cot.float().to(dev)).sum().backward()
    (want * cot).sum().backward()
    assert close(xd.grad, xr.grad, GRAD_TOL), "g_x"
    if eps == 0.0:  # the eps term is skipped: x_0 takes no gradient, on either side
        assert x0d.grad is None and x0r.grad is None
    else:
        assert close(x0d.grad, x0r.grad, GRAD_TOL), "g_x0"
    assert close(conv.att_l.weight.grad, ref.att_l.weight.grad, GRAD_TOL), "g_att_l"
    assert close(conv.att_r.weight.grad, ref.att_r.weight.grad, GRAD_TOL), "g_att_r"
    return out.detach(), xd.grad.detach(), ch


def forms_of(C):
    return ("fused", "composed") if C != REFUSED_WIDTH else ("composed",)


@pytest.mark.parametrize("graph", sorted(GRAPHS))
@pytest.mark.parametrize("C", FUSED_WIDTHS + (REFUSED_WIDTH,))
def test_faconv_eval_forward_backward(dev, C, graph):
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, get_graph
    ei, n = GRAPHS[graph]()
    if graph == "powerlaw":
        g = get_graph(ei.to(dev), n, LOOPS_ADD_REMAINING)
        assert g.fwd.split is not None and g.bwd.split is not None
    assert ops.faconv_supported(C) == (C != REFUSED_WIDTH)
    outs = {form: run_layer(C, ei, n, form, dev, train=False) for form in forms_of(C)}
    if len(outs) == 2:  # fused against composed, both directions, same tolerances as against float64
        (of, gf, _), (oc, gc, _) = outs["fused"], outs["composed"]
        assert close(of, oc.double().cpu(), FWD_TOL) and close(oc, of.double().cpu(), FWD_TOL)
        assert close(gf, gc.double().cpu(), GRAD_TOL) and close(gc, gf.double().cpu(), GRAD_TOL)


@pytest.mark.parametrize("graph", sorted(GRAPHS))
@pytest.mark.parametrize("C", FUSED_WIDTHS + (REFUSED_WIDTH,))
def test_faconv_training_forward_backward(dev, C, graph):
    ei, n = GRAPHS[graph]()
    outs = {form: run_layer(C, ei, n, form, dev, train=True) for form in forms_of(C)}
    if len(outs) == 2:  # the same torch seed gives both forms the same dropout seed, hence the same mask
        (of, gf, chf), (oc, gc, chc) = outs["fused"], outs["composed"]
        assert torch.equal(chf["keep"], chc["keep"])
        assert close(of, oc.double().cpu(), FWD_TOL) and close(oc, of.double().cpu(), FWD_TOL)
        assert close(gf, gc.double().cpu(), GRAD_TOL) and close(gc, gf.double().cpu(), GRAD_TOL)


def test_faconv_eps_zero_and_refused_width(dev):
    ei, n = GRAPHS["random"]()
    run_layer(16, ei, n, "fused", dev, train=False, eps=0.0)
    run_layer(16, ei, n, "composed", dev, train=True, eps=0.0)
    x, x0, ref = make_case(REFUSED_WIDTH, n, 1)
    conv = device_layer(ref, REFUSED_WIDTH, dev, "fused")
    with pytest.raises(RuntimeError, match="composed"):
        conv(x.float().to(dev), x0.float().to(dev), ei.to(dev))


def test_faconv_dropout_draws(dev):
    """Kept share within 5 standard deviations of 1 - p; one seed twice is bit-identical; two seeds differ."""
    ei, n = rand_graph(5000, 40000, 17, loops=5, dups=30), 5000
    x, x0, ref = make_case(16, n, 2, p=0.5)
    conv = device_layer(ref, 16, dev, "fused", p=0.5).train()
    xd, x0d, eid = x.float().to(dev), x0.float().to(dev), ei.to(dev)
    torch.manual_seed(5)
    out_a = conv(xd, x0d, eid)
    ch_a = choices_of(conv, eid, n)
    slots = ch_a["keep"].numel()
    assert slots == int((ei[0] != ei[1]).sum()) + n
    kept = int(ch_a["keep"].sum())
    print(f"kept {kept} of {slots} slots")
    assert abs(kept - 0.5 * slots) <= 5 * (slots * 0.25) ** 0.5, kept
    torch.manual_seed(5)
    out_b = conv(xd, x0d, eid)
    assert torch.equal(out_a, out_b) and torch.equal(ch_a["keep"], choices_of(conv, eid, n)["keep"])
    torch.manual_seed(6)
    out_c = conv(xd, x0d, eid)
    assert not torch.equal(ch_a["keep"], choices_of(conv, eid, n)["keep"]) and not torch.equal(out_a, out_c)
    conv.eval()
    conv(xd, x0d, eid)
    assert conv.last_draw["seed"] is None and bool(choices_of(conv, eid, n)["keep"].all())


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_fagcn_model_against_restatement(dev, p):
    """Logits and every parameter gradient of one training step at 300 nodes; with p = 0.5 the two feature dropouts
    are read off what t1 and the first layer were fed (a float32 normal draw is not exactly 0 unless it was dropped;
    where relu already left a 0 the mask has no effect either way) and the coefficient dropouts off the device."""
    from rgb_experiment_amd.models import FAGCN
    n, f, hid, c = 300, 24, 32, 5
    ei = rand_graph(n, 1800, 31, loops=6, dups=20)
    g = torch.Generator().manual_seed(41)
    x = torch.randn(n, f, generator=g, dtype=torch.float64)
    y = torch.randint(0, c, (n,), generator=g)
    torch.manual_seed(41)
    model = FAGCN(2, f, hid, c, p, 0.3)
    ref = RefFAGCN(2, f, hid, c, p, 0.3)
    ref.load_state_dict({k: v.double() for k, v in model.state_dict().items()}, strict=True)
    model.to(dev).train()
    ref.train()
    eid = ei.to(dev)
    captured = {}
    hooks = [model.t1.register_forward_pre_hook(lambda mod, args: captured.__setitem__("x0", args[0].detach())),
             model.layers[0].register_forward_pre_hook(lambda mod, args: captured.__setitem__("x1", args[0].detach()))]
    torch.manual_seed(9)
    res = model(x.float().to(dev), eid)
    for hk in hooks:
        hk.remove()
    masks = ((captured["x0"] != 0).cpu(), (captured["x1"] != 0).cpu()) if p > 0 else (None, None)
    choices = [choices_of(layer, eid, n) for layer in model.layers] if p > 0 else None
    want = ref(x, ei, choices, masks)
    if p > 0:
        assert abs(masks[0].float().mean().item() - 0.5) < 0.03
        assert all(abs(ch["keep"].float().mean().item() - 0.5) < 0.05 for ch in choices)
        assert not torch.equal(choices[0]["keep"], choices[1]["keep"])  # every layer draws its own seed
    assert close(res["emb"], want["emb"], FWD_TOL) and close(res["out"], want["out"], FWD_TOL)
    torch.nn.functional.nll_loss(res["out"], y.to(dev)).backward()
    torch.nn.functional.nll_loss(want["out"], y).backward()
    refp = dict(ref.named_parameters())
    for name, prm in model.named_parameters():
        assert prm.grad is not None and close(prm.grad, refp[name].grad, GRAD_TOL), name


def planted_partition(n, c, f, seed):
    """c equal blocks; 8 n edges, 85 % inside a block; features = noisy one-hot of the block."""
    import rgb_experiment_amd as R
    g = torch.Generator().manual_seed(seed)
    y = torch.arange(n) % c
    src = torch.randint(0, n, (8 * n,), generator=g)
    inside = torch.rand(8 * n, generator=g) < 0.85
    same = (torch.randint(0, n // c, (8 * n,), generator=g) * c + y[src]) % n
    dst = torch.where(inside, same, torch.randint(0, n, (8 * n,), generator=g))
    x = torch.randn(n, f, generator=g) + 0.8 * torch.nn.functional.one_hot(y, f).float()
    return R.Data(x=x, y=y, edge_index=torch.stack([src, dst]))


def assert_same_run(eager, graphed):
    """The eager loop and the replayed hipGraph computed the same bits. Five of the six curves are formed the same way
    in both loops (float64 sums over float64 counts, divided on the host) and must be EQUAL. The train loss is reported
    differently: the eager loop reads the float32 loss tensor it differentiates (float32(sum / count)), the replay
    divides the same float64 sum and count on the host, so the eager figure must equal the replay's figure rounded to
    float32, exactly. The trained parameters must be equal bit for bit."""
    he, hg = eager["history"], graphed["history"]
    for key in ("val_loss", "test_loss", "train_acc", "val_acc", "test_acc"):
        assert he[key] == hg[key], key
    assert he["train_loss"] == [float(np.float32(v)) for v in hg["train_loss"]]
    sa, sb = eager["model"].state_dict(), graphed["model"].state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_fagcn_experiment_against_a_float64_loop_and_graph_equals_eager(dev):
    import random

    import rgb_experiment_amd as R
    from rgb_experiment_amd.itexperiments import _as_bool_mask, _make_masks
    from rgb_experiment_amd.models import FAGCN
    n, f, c, epochs, lr = 400, 16, 4, 30, 0.01
    data = planted_partition(n, c, f, 5)
    kw = dict(specify_data=True, data=data, model_name="GCN", learning_rate=lr, epoch=epochs, need_to_reappear=True,
              print_print=False, return_model=True, implement_early_stopping=False, need_all_metrics=False)

    def run(p, graphed):
        torch.manual_seed(77)
        model = FAGCN(2, f, 32, c, p, 0.3)
        init = copy.deepcopy(model.state_dict())
        return R.experiment({}, model=model, use_hip_graph="always" if graphed else False, **kw), init

    (eager, init), (graphed, _) = run(0.0, False), run(0.0, True)
    assert graphed["used_hip_graph"] and not eager["used_hip_graph"]
    assert isinstance(eager["model"], FAGCN) and len(eager["history"]["train_loss"]) == epochs
    assert_same_run(eager, graphed)
    # the same 30 epochs in float64 over the restatement (full-batch Adam on the mean NLL of the train rows)
    ref = RefFAGCN(2, f, 32, c, 0.0, 0.3)
    ref.load_state_dict({k: v.double() for k, v in init.items()}, strict=True)
    tm = _as_bool_mask(_make_masks(data.y, "ratio", "6-2-2", 20, 500, 1000, 123456789)[0], n, torch.device("cpu"))
    opt = torch.optim.Adam(ref.parameters(), lr=lr)
    want = []
    x64 = data.x.double()
    for _ in range(epochs):
        ref.train()
        opt.zero_grad()
        loss = torch.nn.functional.nll_loss(ref(x64, data.edge_index)["out"][tm], data.y[tm])
        want.append(loss.item())
        loss.backward()
        opt.step()
    got = eager["history"]["train_loss"]
    worst = max(abs(a - b) for a, b in zip(got, want))
    print(f"loss history: first {got[0]:.6f} / {want[0]:.6f}, last {got[-1]:.6f} / {want[-1]:.6f}, max |diff| {worst:.3e}")
    assert worst < FWD_TOL * max(1.0, max(abs(v) for v in want))
    assert got[-1] < 0.7 * got[0]  # it trains
    # dropout on: the seed is drawn inside the captured epoch and advances with every replay, as in the eager loop
    (eager_d, _), (graphed_d, _) = run(0.5, False), run(0.5, True)
    assert graphed_d["used_hip_graph"]
    assert_same_run(eager_d, graphed_d)
    assert len(set(eager_d["history"]["train_loss"])) == epochs and eager_d["history"]["train_loss"] != got


@pytest.mark.slow
def test_faconv_at_workload_l_on_sampled_rows(dev):
    """|V| = 2 M, |E| = 60 M (bench.py's workload L graph), C = 64, one forward + backward: out and g_x of 64 sampled
    rows against float64 over every edge that touches them (all a row's output and input gradient depend on), with
    the degrees of the whole graph. g_att_l / g_att_r are sums over all nodes and are covered at small sizes."""
    import bench
    from rgb_experiment_amd.nn import FAConv
    wl = bench.WORKLOADS["L"]
    N, C = wl["N"], 64
    ei, x, _ = bench.synth(N, wl["E"], C)
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(N, C, generator=g)
    cot = torch.randn(N, C, generator=g)
    torch.manual_seed(3)
    conv = FAConv(C, eps=0.3).to(dev).eval()
    eid = ei.to(dev)
    xd = x.to(dev).requires_grad_(True)
    out = conv(xd, x0.to(dev), eid)
    (out * cot.to(dev)).sum().backward()
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(9))[:64].to(dev)
    src, dst = eid[0], eid[1]
    hit = torch.zeros(N, dtype=torch.bool, device=dev)
    hit[rows] = True
    touch = hit[dst] | hit[src]
    nodes = torch.unique(torch.cat([rows, src[touch], dst[touch]]))
    local = torch.full((N,), -1, dtype=torch.long, device=dev)
    local[nodes] = torch.arange(nodes.numel(), device=dev)
    sub_ei = torch.stack([local[src[touch]], local[dst[touch]]]).cpu()
    deg = torch.bincount(dst[src != dst], minlength=N) + 1
    ref = RefFAConv(C, eps=0.3).eval()
    ref.load_state_dict({k: v.double().cpu() for k, v in conv.state_dict().items()}, strict=True)
    nc = nodes.cpu()
    xs = x[nc].double().requires_grad_(True)
    want = ref(xs, x0[nc].double(), sub_ei, deg=deg[nodes].cpu())
    (want * cot[nc].double()).sum().backward()
    lr = local[rows].cpu()
    assert close(out[rows], want[lr], FWD_TOL)
    assert close(xd.grad[rows], xs.grad[lr], GRAD_TOL)
