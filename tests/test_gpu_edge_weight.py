"""Edge weights on the MI355X: the weighted graph preparation, every layer / model that takes `edge_weight`, the gradient
with respect to the weights (rgbx_edge_dot_f32 + rgbx_gcn_norm_bwd_f32) and whole experiment() runs, against
oracle/ref_cpu.py composed as gcn_norm(ei, ew, n) [add_loops=False for label propagation] + propagate(..., w).

Tolerances are DESIGN.md section 2's: fp32 outputs within 1e-4 absolute on O(1) data, gradients within
1e-4 * max(1, |g|inf); index arrays bit-exact; the normalised weights within 1e-6 relative. Inputs unless a case says
otherwise: weights U[0.25, 4], features N(0, 1), graphs with accidental duplicate edges and self-loops left in.
Where a gradient is compared the oracle runs in float64, and every such case first checks (`oracle_ok`) that the
float32 oracle itself meets the same bound against its float64 run on the very inputs of the case.
Observed on the CPU for the cases below (fp32 oracle against fp64 oracle): forward maxima between 1.3e-7 (C&S) and
4.2e-6 (APPNP K = 10 on the hub graph; GCNConv 1433 -> 64: 1.8e-6, workload S: 3.5e-7), every gradient below
6e-7 * max(1, |g|inf), the 20-step Adam loss curves within 1e-4 of each other."""

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from test_gpu_ggnn import rand_graph

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4
GRAD_TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def weights(e, seed):
    return torch.rand(e, generator=torch.Generator().manual_seed(seed)) * 3.75 + 0.25


def hub_graph(n, seed):
    """Random edges (duplicates, self-loops) plus a star of 2500 in-edges into node 0 and 1500 out-edges of node 1: rows
    above graph.LONG_ROW_SLOTS = 1024 in the forward AND the transposed CSR."""
    ei = rand_graph(n, 6 * n, seed, loops=7, dups=9)
    g = torch.Generator().manual_seed(seed + 1)
    into = torch.stack([torch.randint(0, n, (2500,), generator=g), torch.zeros(2500, dtype=torch.long)])
    out = torch.stack([torch.ones(1500, dtype=torch.long), torch.randint(0, n, (1500,), generator=g)])
    return torch.cat([ei, into, out], dim=1)


def single_loops(ei, n, k, seed):
    """`ei` without its self-loops plus k self-loops on k DISTINCT nodes (at most one per node)."""
    ei = ei[:, ei[0] != ei[1]]
    nodes = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:k]
    ei = torch.cat([ei, torch.stack([nodes, nodes])], dim=1)
    return ei[:, torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(seed + 1))]


GRAPHS = {"random": lambda: (rand_graph(700, 6000, 3, loops=11, dups=40), 700),
          "hub": lambda: (hub_graph(900, 5), 900)}


def fwd_close(got, want, what=""):
    err = (got.detach().cpu().double() - want.detach().double()).abs().max().item()
    print(f"{what}: max |diff| {err:.3e}, max |ref| {want.detach().abs().max().item():.3e}")
    return err < FWD_TOL


def grad_close(got, want, what=""):
    err = (got.detach().cpu().double() - want.detach().double()).abs().max().item()
    scale = max(1.0, want.detach().abs().max().item())
    print(f"{what}: max |diff| {err:.3e}, |g|inf {scale:.3e}")
    return err < GRAD_TOL * scale


def ref_conv(x, ei, ew, weight, bias, add_loops=True):
    n = x.size(0)
    ei2, w = O.gcn_norm(ei, ew, n, add_loops=add_loops, dtype=x.dtype)
    out = O.propagate(ei2, x @ weight.t(), n, w)
    return out if bias is None else out + bias


def ref_appnp(x, ei, ew, K, alpha):
    n = x.size(0)
    ei2, w = O.gcn_norm(ei, ew, n, dtype=x.dtype)
    z = x
    for _ in range(K):
        z = (1 - alpha) * O.propagate(ei2, z, n, w) + alpha * x
    return z


def ref_gcn(sd, x, ei, ew, training):
    h = ref_conv(x, ei, ew, sd["convs.0.lin.weight"], sd["convs.0.bias"])
    h = O.batch_norm(h, sd, "bns.0.", training)
    return ref_conv(h, ei, ew, sd["convs.1.lin.weight"], sd["convs.1.bias"])


def ref_label_propagation(y, ei, ew, layers, alpha, post_step=None):
    post_step = post_step or (lambda t: t.clamp_(0.0, 1.0))
    n = y.size(0)
    _, w = O.gcn_norm(ei, ew, n, add_loops=False, dtype=y.dtype)
    out, res = y, (1 - alpha) * y
    for _ in range(layers):
        out = post_step(O.propagate(ei, out, n, w) * alpha + res)
    return out


def oracle_ok(fn, tensors, grads=True):
    """The float32 oracle against its float64 run under the test's own bounds; returns the float64 outputs:
    (out, [grad per tensor that requires grad])."""
    res = {}
    for dt in (torch.float32, torch.float64):
        leaves = [t.detach().to(dt).requires_grad_(t.requires_grad) if t.is_floating_point() else t for t in tensors]
        out = fn(*leaves)
        gs = []
        if grads:
            want = [t for t in leaves if t.is_floating_point() and t.requires_grad]
            gs = list(torch.autograd.grad(out.square().sum() * 0.5 / out.size(0), want))
        res[dt] = (out.detach(), gs)
    assert fwd_close(res[torch.float32][0], res[torch.float64][0], "oracle fp32 vs fp64")
    for a, b in zip(res[torch.float32][1], res[torch.float64][1]):
        assert grad_close(a, b, "oracle grad fp32 vs fp64")
    return res[torch.float64]


def loss_of(out):
    return out.square().sum() * 0.5 / out.size(0)


# ---- unit weights -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(GRAPHS))
def test_unit_weights_are_bit_identical_to_the_unweighted_call(dev, name):
    from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, LOOPS_KEEP, LOOPS_REMOVE_ADD, get_graph
    from rgb_experiment_amd.nn import APPNP, GCNConv
    ei, n = GRAPHS[name]()
    eid = ei.to(dev)
    ones = torch.ones(ei.size(1), device=dev)
    for mode in (LOOPS_KEEP, LOOPS_ADD_REMAINING, LOOPS_REMOVE_ADD):
        a, b = get_graph(eid, n, mode), get_graph(eid, n, mode, ones)
        assert b is not a and b.fwd is a.fwd and b.bwd is a.bwd  # the sort did not run twice
        if name == "hub":
            assert a.fwd.split is not None and a.bwd.split is not None
        for attr in ("dis", "w", "w_t"):
            assert torch.equal(getattr(a, attr), getattr(b, attr)), (mode, attr)
        assert torch.equal(a.rowsum("gcn"), b.rowsum("gcn"))
    assert get_graph(eid, n, LOOPS_ADD_REMAINING, ones) is get_graph(eid, n, LOOPS_ADD_REMAINING, ones)
    g = torch.Generator().manual_seed(1)
    for fin, fout in ((128, 128), (64, 7)):
        x = torch.randn(n, fin, generator=g).to(dev)
        torch.manual_seed(3)
        conv = GCNConv(fin, fout).to(dev)
        with torch.no_grad():
            assert torch.equal(conv(x, eid), conv(x, eid, ones))
        xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        loss_of(conv(xa, eid)).backward()
        ga = conv.lin.weight.grad.clone()
        conv.zero_grad()
        loss_of(conv(xb, eid, ones)).backward()
        assert torch.equal(ga, conv.lin.weight.grad) and torch.equal(xa.grad, xb.grad)
    h = torch.randn(n, 8, generator=g).to(dev)
    assert torch.equal(APPNP(10, 0.1)(h, eid), APPNP(10, 0.1)(h, eid, ones))


# ---- weighted gcn_norm --------------------------------------------------------------------------------------------------

def two_loop_graph():
    """Node 2 has TWO input self-loops (edge 1: weight 3, edge 4: weight 0.5 — the last one wins), node 0 one, node 3 none."""
    ei = torch.tensor([[0, 2, 1, 0, 2, 3, 1], [1, 2, 2, 0, 2, 1, 3]])
    ew = torch.tensor([2.0, 3.0, 0.25, 4.0, 0.5, 1.5, 1.0])
    return ei, ew, 4


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", ["random", "hub", "two_loops"])
def test_weighted_gcn_norm_matches_the_oracle(dev, name, mode):
    from rgb_experiment_amd.graph import get_graph
    if name == "two_loops":
        ei, ew, n = two_loop_graph()
    else:
        ei, n = GRAPHS[name]()
        ew = weights(ei.size(1), 17)
    E = ei.size(1)
    if mode == 0:
        ref_ei, ref_ew = ei, ew
    elif mode == 1:
        ref_ei, ref_ew = O.add_remaining_self_loops(ei, ew, 1.0, n)
    else:
        ref_ei, ref_ew = O.add_self_loops(*O.remove_self_loops(ei, ew), 1.0, n)
    _, ref_w = O.gcn_norm(ref_ei, ref_ew.double(), n, add_loops=False, dtype=torch.float64)
    _, ids = O.rewrite_edges(ei, n, mode)  # rewritten edge -> id (input edge, or E + node for an added loop)
    by_id = torch.full((E + n,), float("nan"), dtype=torch.float64)
    by_id[ids] = ref_w
    g = get_graph(ei.to(dev), n, mode, ew.to(dev))
    for csr, w in ((g.fwd, g.w), (g.bwd, g.w_t)):
        rowptr, col, perm = O.csr_from_edges(ref_ei[1] if csr is g.fwd else ref_ei[0],
                                             ref_ei[0] if csr is g.fwd else ref_ei[1], ids, n)
        assert torch.equal(csr.rowptr.cpu(), rowptr) and torch.equal(csr.col[:csr.nnz].cpu(), col)
        assert torch.equal(csr.perm[:csr.nnz].cpu(), perm)
        got = torch.full((E + n,), float("nan"), dtype=torch.float64)
        got[csr.perm[:csr.nnz].cpu().long()] = w[:csr.nnz].cpu().double()
        assert torch.equal(got.isnan(), by_id.isnan())
        zero = by_id == 0  # a source without in-edges has dis = 0 (inf -> 0): exactly 0 on both sides
        assert bool((got[zero] == 0).all())
        used = ~by_id.isnan() & ~zero
        rel = ((got[used] - by_id[used]).abs() / by_id[used].abs()).max().item()
        print(f"{name} mode {mode}: max relative error of w {rel:.3e}")
        assert rel < 1e-6


def test_two_self_loops_known_answer(dev):
    """Hand-derived: after add_remaining_self_loops the loops weigh [4 (edge 3), 1 (filled), 0.5 (edge 4, the LAST of node
    2's two), 1 (filled)]; weighted in-degrees: node 0: 4; node 1: 2 + 1.5 + 1 = 4.5; node 2: 0.25 + 0.5 = 0.75;
    node 3: 1 + 1 = 2."""
    from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, get_graph
    ei, ew, n = two_loop_graph()
    g = get_graph(ei.to(dev), n, LOOPS_ADD_REMAINING, ew.to(dev))
    loop_w, loop_src = g.loops
    assert loop_w.cpu().tolist() == [4.0, 1.0, 0.5, 1.0]
    assert loop_src.cpu().tolist() == [3, -1, 4, -1]
    deg = torch.tensor([4.0, 4.5, 0.75, 2.0], dtype=torch.float64)
    assert torch.allclose(g.dis.cpu().double(), deg.pow(-0.5), rtol=1e-6, atol=0)
    dis = deg.pow(-0.5)
    # forward slots: row 0: loop; row 1: edges 0 (0->1), 5 (3->1), loop; row 2: edge 2 (1->2), loop; row 3: edge 6, loop
    assert g.fwd.perm[:g.fwd.nnz].cpu().tolist() == [7, 0, 5, 8, 2, 9, 6, 10]
    want = torch.stack([dis[0] * 4 * dis[0], dis[0] * 2 * dis[1], dis[3] * 1.5 * dis[1], dis[1] * 1 * dis[1],
                        dis[1] * 0.25 * dis[2], dis[2] * 0.5 * dis[2], dis[1] * 1 * dis[3], dis[3] * 1 * dis[3]])
    assert torch.allclose(g.w[:g.fwd.nnz].cpu().double(), want, rtol=1e-6, atol=0)


def test_weight_contract_on_the_device(dev):
    from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, get_graph
    ei, n = GRAPHS["random"]()
    eid, ew = ei.to(dev), weights(ei.size(1), 2).to(dev)
    with pytest.raises(ValueError, match="is on"):
        get_graph(eid, n, LOOPS_ADD_REMAINING, ew.cpu())
    bad = ew.clone()
    bad[5] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        get_graph(eid, n, LOOPS_ADD_REMAINING, bad)
    g = get_graph(eid, n, LOOPS_ADD_REMAINING, ew)
    with pytest.raises(RuntimeError, match="mean"):
        g.inv_deg
    with pytest.raises(RuntimeError, match="mean"):
        g.w_mean_t
    ew.mul_(2.0)  # an in-place edit moves the version: a new entry
    assert get_graph(eid, n, LOOPS_ADD_REMAINING, ew) is not g


# ---- layers and models --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fin,fout", [(128, 128), (1433, 64), (64, 7)])
def test_gcnconv_forward_and_gradients(dev, fin, fout):
    from rgb_experiment_amd.nn import GCNConv
    ei, n = GRAPHS["random"]()
    ew = weights(ei.size(1), 21)
    x = torch.randn(n, fin, generator=torch.Generator().manual_seed(4)).requires_grad_(True)
    torch.manual_seed(8)
    conv = GCNConv(fin, fout)
    with torch.no_grad():
        conv.bias.uniform_(-0.5, 0.5)
    W, b = conv.lin.weight.detach().clone().requires_grad_(True), conv.bias.detach().clone().requires_grad_(True)
    want, (gx, gW, gb) = oracle_ok(lambda x_, W_, b_: ref_conv(x_, ei, ew.to(x_.dtype), W_, b_), [x, W, b])
    conv.to(dev)
    xd = x.detach().to(dev).requires_grad_(True)
    out = conv(xd, ei.to(dev), ew.to(dev))
    loss_of(out).backward()
    assert fwd_close(out, want, "out")
    assert grad_close(xd.grad, gx, "x.grad") and grad_close(conv.lin.weight.grad, gW, "dW")
    assert grad_close(conv.bias.grad, gb, "db")
    with torch.no_grad():  # the input-layer route (x needs no gradient) and the eval route
        assert fwd_close(conv(xd.detach(), ei.to(dev), ew.to(dev)), want, "no_grad out")


def _gcn(dev, fin=48, hid=128, C=7, seed=12):
    from rgb_experiment_amd.models import GCN
    torch.manual_seed(seed)
    net = GCN(num_layers=2, hidden_unit=hid, input_dim=fin, output_dim=C, dropout_rate=0.5)
    with torch.no_grad():
        for conv in net.convs:
            conv.bias.uniform_(-0.2, 0.2)
        net.bns[0].weight.uniform_(0.5, 1.5)
        net.bns[0].bias.uniform_(-0.2, 0.2)
        net.bns[0].running_mean.uniform_(-0.2, 0.2)
        net.bns[0].running_var.uniform_(0.5, 1.5)
    return net


@pytest.mark.parametrize("hid", [128, 64])
def test_gcn_model_train_and_eval(dev, hid):
    ei, n = GRAPHS["random"]()
    ew = weights(ei.size(1), 23)
    x = torch.randn(n, 48, generator=torch.Generator().manual_seed(6))
    net = _gcn(dev, hid=hid)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    names = [k for k, _ in net.named_parameters()]
    params = [sd[k].clone().requires_grad_(True) for k in names]

    def ref(training):
        def fn(*ps):
            d = dict(sd)
            d.update({k: p for k, p in zip(names, ps)})
            d = {k: (v.to(ps[0].dtype) if v.is_floating_point() else v) for k, v in d.items()}
            return ref_gcn(d, x.to(ps[0].dtype), ei, ew.to(ps[0].dtype), training)
        return fn

    want_train, grads = oracle_ok(ref(True), params)
    want_eval, _ = oracle_ok(ref(False), params, grads=False)
    net.to(dev)
    xd, eid, ewd = x.to(dev), ei.to(dev), ew.to(dev)
    net.train()
    out = net(xd, eid, ewd)["emb"]
    loss_of(out).backward()
    assert fwd_close(out, want_train, "train logits")
    for k, p, g in zip(names, net.parameters(), grads):
        assert grad_close(p.grad, g, k)
    net.load_state_dict({k: v.to(dev) for k, v in sd.items()})  # the training forward moved the running statistics
    net.eval()
    outs = {}
    with torch.no_grad():
        for label, collapse, cache in (("collapsed", True, False), ("layerwise", False, False), ("cached", False, True)):
            net.collapse_eval, net.cache_input_aggregate = collapse, cache
            outs[label] = net(xd, eid, edge_weight=ewd)["emb"]
            assert fwd_close(outs[label], want_eval, f"eval logits ({label})")
    assert fwd_close(outs["collapsed"], outs["layerwise"].cpu(), "collapsed vs layerwise")
    assert fwd_close(outs["cached"], outs["layerwise"].cpu(), "cached vs layerwise")
    y = torch.randint(0, 7, (n,), generator=torch.Generator().manual_seed(2)).to(dev)
    mask = (torch.rand(n, generator=torch.Generator().manual_seed(3)) < 0.4).to(dev)
    with torch.no_grad():  # the loss-in-kernel forms on the weighted graph
        net.collapse_eval, net.cache_input_aggregate = True, False
        _, stats = net.masked_ce(xd, eid, y, mask, edge_weight=ewd)
    ref_nll = F.nll_loss(torch.log_softmax(want_eval, 1)[mask.cpu()], y.cpu()[mask.cpu()], reduction="sum").item()
    assert abs(stats[0].item() - ref_nll) < FWD_TOL * max(1.0, abs(ref_nll))


def test_appnp_and_sgconv(dev):
    from rgb_experiment_amd.nn import APPNP, SGConv
    ei, n = GRAPHS["hub"]()
    ew = weights(ei.size(1), 27)
    x = torch.randn(n, 8, generator=torch.Generator().manual_seed(9)).requires_grad_(True)
    want, (gx,) = oracle_ok(lambda x_: ref_appnp(x_, ei, ew.to(x_.dtype), 10, 0.1), [x])
    xd = x.detach().to(dev).requires_grad_(True)
    out = APPNP(10, 0.1)(xd, ei.to(dev), ew.to(dev))
    loss_of(out).backward()
    assert fwd_close(out, want, "APPNP out") and grad_close(xd.grad, gx, "APPNP x.grad")

    for fin, fout, loops in ((40, 7, True), (8, 16, True), (8, 16, False)):
        torch.manual_seed(5)
        conv = SGConv(fin, fout, K=2, add_self_loops=loops)
        x = torch.randn(n, fin, generator=torch.Generator().manual_seed(10)).requires_grad_(True)
        W, b = conv.lin.weight.detach().clone().requires_grad_(True), conv.lin.bias.detach().clone().requires_grad_(True)

        def ref(x_, W_, b_):
            ei2, w = O.gcn_norm(ei, ew.to(x_.dtype), n, add_loops=loops, dtype=x_.dtype)
            h = x_
            for _ in range(2):
                h = O.propagate(ei2, h, n, w)
            return h @ W_.t() + b_

        want, (gx, gW, gb) = oracle_ok(ref, [x, W, b])
        conv.to(dev)
        xd = x.detach().to(dev).requires_grad_(True)
        out = conv(xd, ei.to(dev), ew.to(dev))
        loss_of(out).backward()
        assert fwd_close(out, want, "SGConv out") and grad_close(xd.grad, gx, "SGConv x.grad")
        assert grad_close(conv.lin.weight.grad, gW, "SGConv dW") and grad_close(conv.lin.bias.grad, gb, "SGConv db")
    cached = SGConv(8, 16, K=2, cached=True).to(dev)
    with torch.no_grad():
        first = cached(xd.detach(), ei.to(dev), ew.to(dev))
        again = cached(xd.detach(), ei.to(dev), torch.ones_like(ew).to(dev))  # keyed to the first call's weights
    assert torch.equal(first, again)


def test_correct_and_smooth(dev):
    from rgb_experiment_amd.initial_params import InitialParameters
    from rgb_experiment_amd.nn import CorrectAndSmooth
    ei, n = GRAPHS["random"]()
    ew = weights(ei.size(1), 31)
    g = torch.Generator().manual_seed(13)
    C = 5
    y_soft = torch.softmax(torch.randn(n, C, generator=g), 1)
    y = torch.randint(0, C, (n,), generator=g)
    mask = torch.rand(n, generator=g) < 0.3
    p = InitialParameters.default_cs_param

    def ref(dt):
        ys, w = y_soft.to(dt), ew.to(dt)
        onehot = F.one_hot(y[mask], C).to(dt)
        error = torch.zeros_like(ys)
        error[mask] = onehot - ys[mask]
        sm = ref_label_propagation(error, ei, w, p["num_correction_layers"], p["correction_alpha"],
                                   lambda t: t.clamp_(-1.0, 1.0))
        sc = (error[mask].abs().sum() / int(mask.sum())) / sm.abs().sum(dim=1, keepdim=True)
        sc[sc.isinf() | (sc > 1000)] = 1.0
        out = (ys + sc * sm).clone()
        out[mask] = onehot
        return ref_label_propagation(out, ei, w, p["num_smoothing_layers"], p["smoothing_alpha"])

    want = ref(torch.float64)
    assert fwd_close(ref(torch.float32), want, "oracle fp32 vs fp64")
    post = CorrectAndSmooth(**p)
    d = lambda t: t.to(dev)
    got = post.correct(d(y_soft), d(y[mask]), d(mask), d(ei), d(ew))
    got = post.smooth(got, d(y[mask]), d(mask), d(ei), edge_weight=d(ew))
    assert fwd_close(got, want, "C&S")


def test_workload_s_on_sampled_rows(dev):
    """GCNConv 128 -> 128 (the fused kernel) at workload S's graph: N = 200 000, E = 4 000 000. The oracle's gcn_norm runs
    on the WHOLE graph (vectors of E' entries); its propagate on the in-edges of 256 sampled targets only."""
    from oracle.sampled import pick_targets
    from rgb_experiment_amd.nn import GCNConv
    n, e, d = 200_000, 4_000_000, 128
    g = torch.Generator().manual_seed(77)
    ei = torch.randint(0, n, (2, e), generator=g)
    ew = weights(e, 78)
    x = torch.randn(n, d, generator=g)
    torch.manual_seed(4)
    conv = GCNConv(d, d)
    targets = pick_targets(n, 256)
    flag = torch.zeros(n, dtype=torch.bool)
    flag[targets] = True
    outs = {}
    for dt in (torch.float32, torch.float64):
        ei2, w = O.gcn_norm(ei, ew.to(dt), n, dtype=dt)
        keep = flag[ei2[1]]
        nodes = torch.cat([ei2[0][keep], targets]).unique()
        pos = torch.full((n,), -1, dtype=torch.int64)
        pos[nodes] = torch.arange(nodes.numel())
        sub = torch.stack([pos[ei2[0][keep]], pos[ei2[1][keep]]])
        h = x[nodes].to(dt) @ conv.lin.weight.detach().to(dt).t()
        outs[dt] = (O.propagate(sub, h, nodes.numel(), w[keep]) + conv.bias.detach().to(dt))[pos[targets]]
    assert fwd_close(outs[torch.float32], outs[torch.float64], "oracle fp32 vs fp64")
    conv.to(dev)
    with torch.no_grad():
        got = conv(x.to(dev), ei.to(dev), ew.to(dev))[targets.to(dev)]
    assert fwd_close(got, outs[torch.float64], "workload S, 256 sampled rows")


# ---- edge_weight.requires_grad ------------------------------------------------------------------------------------------

GRAD_GRAPHS = {"random": lambda: (single_loops(rand_graph(700, 6000, 3, dups=40), 700, 60, 8), 700),
               "hub": lambda: (single_loops(hub_graph(900, 5), 900, 80, 9), 900)}


@pytest.mark.parametrize("d", [4, 8, 64, 128, 256, 7, 300])
@pytest.mark.parametrize("name", list(GRAD_GRAPHS))
def test_edge_dot_slot_by_slot(dev, name, d):
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, get_graph
    ei, n = GRAD_GRAPHS[name]()
    graph = get_graph(ei.to(dev), n, LOOPS_ADD_REMAINING)
    g = torch.Generator().manual_seed(d)
    a, b = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    for csr in (graph.fwd, graph.bwd):
        if name == "hub":
            assert csr.split is not None
        got = ops.edge_dot_raw(csr, a.to(dev), b.to(dev))[:csr.nnz]
        rows = torch.repeat_interleave(torch.arange(n), (csr.rowptr[1:] - csr.rowptr[:-1]).cpu().long())
        want = (a.double()[rows] * b.double()[csr.col[:csr.nnz].cpu().long()]).sum(1)
        assert grad_close(got, want, f"edge dot d={d}")  # |g|inf ~ 4 sqrt(d)
        assert torch.equal(got, ops.edge_dot_raw(csr, a.to(dev), b.to(dev))[:csr.nnz])  # same bits twice


@pytest.mark.parametrize("fin,fout", [(32, 64), (64, 7)])
@pytest.mark.parametrize("name", list(GRAD_GRAPHS))
def test_gradient_in_the_edge_weights(dev, name, fin, fout):
    from rgb_experiment_amd.nn import GCNConv
    ei, n = GRAD_GRAPHS[name]()
    ew = weights(ei.size(1), 41).requires_grad_(True)
    x = torch.randn(n, fin, generator=torch.Generator().manual_seed(14)).requires_grad_(True)
    torch.manual_seed(15)
    conv = GCNConv(fin, fout)
    W, b = conv.lin.weight.detach().clone().requires_grad_(True), conv.bias.detach().clone().requires_grad_(True)
    want, (gx, gew, gW, gb) = oracle_ok(lambda x_, ew_, W_, b_: ref_conv(x_, ei, ew_, W_, b_), [x, ew, W, b])
    conv.to(dev)
    xd = x.detach().to(dev).requires_grad_(True)
    ewd = ew.detach().to(dev).requires_grad_(True)
    out = conv(xd, ei.to(dev), ewd)
    loss_of(out).backward()
    assert fwd_close(out, want, "out")
    assert grad_close(ewd.grad, gew, "edge_weight.grad")
    assert grad_close(xd.grad, gx, "x.grad") and grad_close(conv.lin.weight.grad, gW, "dW")
    assert grad_close(conv.bias.grad, gb, "db")


def test_learnable_mask_adam_run(dev):
    """20 Adam steps over mask logits m (edge_weight = 4 sigmoid(m)) through a 2-layer GCN with fixed parameters: the loss
    falls, and the curve is the float64 oracle's within 1e-4."""
    ei, n = GRAD_GRAPHS["random"]()
    x = torch.randn(n, 48, generator=torch.Generator().manual_seed(6))
    y = torch.randint(0, 7, (n,), generator=torch.Generator().manual_seed(7))
    net = _gcn(dev, hid=64).eval()
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    m0 = torch.randn(ei.size(1), generator=torch.Generator().manual_seed(16)) * 0.5

    def run(forward, m, y_):
        opt = torch.optim.Adam([m], lr=0.1)
        curve = []
        for _ in range(20):
            opt.zero_grad()
            loss = F.nll_loss(torch.log_softmax(forward(4 * torch.sigmoid(m)), 1), y_)
            loss.backward()
            opt.step()
            curve.append(loss.item())
        return curve

    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    ref = run(lambda w: ref_gcn(sd64, x.double(), ei, w, False), m0.double().requires_grad_(True), y)
    sd32 = {k: v for k, v in sd.items()}
    ref32 = run(lambda w: ref_gcn(sd32, x, ei, w, False), m0.clone().requires_grad_(True), y)
    assert max(abs(a - b) for a, b in zip(ref32, ref)) < 1e-4  # the oracle's own fp32 run meets the bound
    net.to(dev)
    for p in net.parameters():
        p.requires_grad_(False)
    xd, eid = x.to(dev), ei.to(dev)
    got = run(lambda w: net(xd, eid, edge_weight=w)["emb"], m0.to(dev).requires_grad_(True), y.to(dev))
    print("loss curve", [f"{v:.5f}" for v in got], "max |diff|", max(abs(a - b) for a, b in zip(got, ref)))
    assert got[-1] < got[0] - 1e-3
    assert max(abs(a - b) for a, b in zip(got, ref)) < 1e-4


# ---- whole runs ---------------------------------------------------------------------------------------------------------

def _data(with_weight=True):
    from rgb_experiment_amd.data import Data
    g = torch.Generator().manual_seed(5)
    n, e = 600, 5000
    extra = {"edge_weight": weights(e, 51)} if with_weight else {}
    y = torch.randint(0, 4, (n,), generator=g)
    x = torch.randn(n, 24, generator=g) + F.one_hot(y, 24).float() * 1.5
    return Data(x=x, y=y, edge_index=torch.randint(0, n, (2, e), generator=g), **extra)


def _run(data, **kw):
    from rgb_experiment_amd import experiment
    args = dict(specify_data=True, data=data, remake_data_mask=True, epoch=6, print_print=False, return_model=True,
                need_to_reappear=True, model_name="gcn", learning_rate=0.01, implement_early_stopping=False)
    args.update(kw)
    init = args.pop("init", {"num_layers": 2, "hidden_unit": 64, "dropout_rate": 0.5})
    return experiment(init, **args)


def test_experiment_weighted_eager_and_hipgraph_agree(dev):
    eager = _run(_data(), use_edge_weight=True, use_hip_graph=False)
    graphed = _run(_data(), use_edge_weight=True, use_hip_graph=True)
    assert graphed["used_hip_graph"] and not eager["used_hip_graph"]
    for k in ("train_loss", "train_acc", "val_loss", "val_acc", "test_acc"):
        assert len(eager["history"][k]) == 6
        assert eager["history"][k] == pytest.approx(graphed["history"][k], abs=1e-6), k
    plain = _run(_data(), use_edge_weight=False, use_hip_graph=False)
    assert plain["history"]["train_loss"] != eager["history"]["train_loss"]  # the weights are in the arithmetic
    for name, init in (("appnpstack", {"hidden_unit": 16, "K": 3, "alpha": 0.1, "dropout_rate": 0.5}),
                       ("sgc", {"K": 2})):
        res = _run(_data(), model_name=name, init=init, use_edge_weight=True, post_cs=name == "sgc")
        assert 0.0 <= res["ACC"] <= 1.0


def test_experiment_without_the_flag_is_unchanged(dev):
    for graph in (False, True):
        a = _run(_data(False), use_hip_graph=graph)
        b = _run(_data(True), use_hip_graph=graph)
        assert a["history"] == b["history"] and a["ACC"] == b["ACC"]
