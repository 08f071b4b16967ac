"""The softmax and log-sum-exp kernels on the MI355X at trained score ranges: attention scores of several hundred and
logits of +-150 and beyond, where the online-softmax rescale, the merge of (max, sum, accumulator) states with unequal
maxima, the start value of the running maximum, the (max, 1 / sum) record the backward passes read and the loss
kernels' exp(z - lse) do arithmetic that scores of order 1 never reach.

The cases, the references and the proof that each case is in that regime AND well-posed in float32 are in
tests/test_softmax_range_host.py (no GPU). Tolerances are the project's, unchanged: forward 1e-4 * max(1, |ref|max),
gradients 2e-4 * max(1, |ref|max) through `close`, every element compared, every output and gradient finite; the
per-edge softmax within 1e-6 absolute; the loss: NLL sum within 1e-5 * max(1, |ref|), counts exact, gradient within
1e-6 absolute."""
import pytest
import torch

import test_softmax_range_host as R
from test_gpu_ggnn import close
from test_softmax_range_host import FWD_TOL, GRAD_TOL, SLOPE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def device_graph(name, dev):
    from rgb_experiment_amd.graph import LOOPS_REMOVE_ADD, get_graph
    ei, n = R.graph_of(name)
    graph = get_graph(ei.to(dev), n, LOOPS_REMOVE_ADD)
    if name != "random":
        assert graph.fwd.split is not None      # the chunk + combine kernels of the forward run
    if name == "powerlaw":
        assert graph.bwd.split is not None      # and those of the pass over the transposed CSR
    return graph


def finite(*tensors):
    return all(bool(torch.isfinite(t).all()) for t in tensors)


def check(got, want, names):
    """got / want = (out, [gradients]); `names` as in the host module: forward first."""
    assert finite(got[0], *got[1]), "non-finite output or gradient"
    assert got[0].shape == want[0].shape and close(got[0], want[0], FWD_TOL), names[0]
    for name, a, b in zip(names[1:], got[1], want[1]):
        assert a.shape == b.shape and close(a, b, GRAD_TOL), name


def leaf(t, dev):
    return t.float().to(dev).requires_grad_(True)


# ---- GATv2 ------------------------------------------------------------------------------------------------------------

def run_gatv2(H, C, graph_name, dev, train, torch_seed=5):
    from rgb_experiment_amd import ops
    from test_gpu_gatv2 import choices_of
    graph = device_graph(graph_name, dev)
    p = 0.5 if train else 0.0
    xl, xr, att, bias, cot = R.gatv2_case(H, C, graph_name)
    xl_d, xr_d, att_d, bias_d = (leaf(t, dev) for t in (xl, xr, att, bias))
    record = {}
    torch.manual_seed(torch_seed)
    out = ops.gatv2_attend(xl_d, xr_d, att_d, graph, H, C, SLOPE, bias=bias_d, training=train, p_drop=p, record=record)
    (out * cot.float().to(dev)).sum().backward()
    got = (out.detach(), [xl_d.grad, xr_d.grad, att_d.grad, bias_d.grad])
    if train:
        ch = choices_of(record, graph, H)
        assert record["seed"] is not None and ch["keep"].shape == (ch["src"].numel(), H)
        want = R.gatv2_reference(H, C, graph_name, ch["src"], ch["dst"], ch["keep"], p)
    else:
        assert record["seed"] is None
        want = R.gatv2_eval_reference(H, C, graph_name)
    check(got, want, R.GATV2_NAMES)
    return got


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("graph", R.GATV2_GRAPHS)
@pytest.mark.parametrize("H,C", R.GATV2_PAIRS)
def test_gatv2_attend(dev, H, C, graph, train):
    run_gatv2(H, C, graph, dev, train)


# ---- GAT --------------------------------------------------------------------------------------------------------------

def run_gat_aggregate(H, C, graph_name, dev):
    from rgb_experiment_amd import ops
    graph = device_graph(graph_name, dev)
    h, a_src, a_dst, cot = R.gat_case(H, C, graph_name)
    h_d, as_d, ad_d = (leaf(t, dev) for t in (h, a_src, a_dst))
    out = ops.gat_aggregate(h_d, as_d, ad_d, graph, H, C, SLOPE)
    (out * cot.float().to(dev)).sum().backward()
    got = (out.detach(), [h_d.grad, as_d.grad, ad_d.grad])
    check(got, R.gat_reference(H, C, graph_name), R.GAT_NAMES)
    with torch.no_grad():  # the inference form (no positive-score parts stored, one more neighbour row in flight)
        plain = ops.gat_aggregate(h_d.detach(), as_d.detach(), ad_d.detach(), graph, H, C, SLOPE)
    assert finite(plain) and close(plain, R.gat_reference(H, C, graph_name)[0], FWD_TOL), "inference form"
    return got


@pytest.mark.parametrize("graph", R.GAT_GRAPHS)
@pytest.mark.parametrize("H,C", R.GAT_PAIRS)
def test_gat_aggregate(dev, H, C, graph):
    run_gat_aggregate(H, C, graph, dev)


@pytest.mark.parametrize("graph", R.GAT_ATTEND_GRAPHS)
@pytest.mark.parametrize("H,C", R.GAT_ATTEND_PAIRS)
def test_gat_attend(dev, H, C, graph):
    """Scores formed inside the aggregation kernel (C = 16) and by the scores launch (C = 128)."""
    from rgb_experiment_amd import ops
    assert ops._scores_in_kernel(C) == (C == 16)
    graph_d = device_graph(graph, dev)
    h, att_src, att_dst, bias, cot = R.gat_attend_case(H, C, graph)
    h_d, s_d, d_d, b_d = (leaf(t, dev) for t in (h, att_src, att_dst, bias))
    out = ops.gat_attend(h_d, s_d, d_d, graph_d, H, C, SLOPE, bias=b_d)
    (out * cot.float().to(dev)).sum().backward()
    check((out.detach(), [h_d.grad, s_d.grad, d_d.grad, b_d.grad]), R.gat_attend_reference(H, C, graph), R.GAT_ATTEND_NAMES)
    with torch.no_grad():
        plain = ops.gat_attend(h_d.detach(), s_d.detach(), d_d.detach(), graph_d, H, C, SLOPE, bias=b_d.detach())
    assert finite(plain) and close(plain, R.gat_attend_reference(H, C, graph)[0], FWD_TOL), "inference form"


def test_gat_edge_softmax_on_the_hub_graph(dev):
    """The row kernel and the hub-row kernel of rgbx_gat_edge_softmax_f32, edge by edge in slot order."""
    from rgb_experiment_amd import ops
    graph = device_graph("hub", dev)
    _, n = R.graph_of("hub")
    a_src, a_dst = R.edge_softmax_case()
    want_alpha, want_pos, want_apos, want_m, _ = R.edge_softmax_formula(a_src, a_dst)
    args = (graph.fwd, a_src.float().to(dev), a_dst.float().to(dev), R.EDGE_SOFTMAX_SLOPE)
    alpha, alpha_pos, m, rden, a_pos = ops.gat_edge_softmax(*args, True, n)
    assert finite(alpha, alpha_pos, m, rden, a_pos)
    assert alpha.numel() == want_alpha.numel()
    assert (alpha.cpu().double() - want_alpha).abs().max().item() < 1e-6
    assert (alpha_pos.cpu().double() - want_pos).abs().max().item() < 1e-6
    assert close(a_pos, want_apos, FWD_TOL)
    assert torch.equal(m.cpu().double(), want_m)  # the scores are exact in float32, so is their maximum
    again = ops.gat_edge_softmax(*args, False, n)
    assert torch.equal(alpha, again[0]) and again[1] is None and torch.equal(m, again[2]) and torch.equal(rden, again[3])


def test_gat_attend_linear_forward(dev):
    """The single-head aggregate-first form: per-edge coefficients from the edge-softmax kernel, then the fused layer."""
    from rgb_experiment_amd import ops
    graph = device_graph("hub", dev)
    ei, n = R.graph_of("hub")
    case = R.gat_linear_case("hub")
    x, W, att_src, att_dst, bias = (t.float().to(dev) for t in case)
    assert ops.gat_linear_ok(graph, R.GAT_LINEAR_F, R.GAT_LINEAR_C, x)
    want, _ = R.gat_linear_formula(*case, ei)
    out = ops.gat_attend_linear(x.clone().requires_grad_(True), W, att_src, att_dst, graph, SLOPE, bias=bias)
    assert finite(out) and close(out, want, FWD_TOL), "the form that prepares a backward"
    with torch.no_grad():
        plain = ops.gat_attend_linear(x, W, att_src, att_dst, graph, SLOPE, bias=bias)
    assert finite(plain) and close(plain, want, FWD_TOL), "inference form"


# ---- SuperGAT ---------------------------------------------------------------------------------------------------------

def run_supergat(H, C, concat, graph_name, dev, train, lin_scale=1.0, torch_seed=5):
    """tests/test_gpu_supergat.py's run_eval / run_train on a scaled case."""
    from test_gpu_supergat import assert_no_kink, choices_of, device_layer
    ei, n = R.graph_of(graph_name)
    device_graph(graph_name, dev)
    p = 0.6 if train else 0.0
    x, ref = R.supergat_case(H, C, concat, graph_name, p=p, lin_scale=lin_scale)
    conv = device_layer(ref, x.size(1), dev, p=p, ratios=(0.8, 0.5) if train else (1.0, 0.5)).train(train)
    xd = leaf(x, dev)
    eid = ei.to(dev)
    torch.manual_seed(torch_seed)
    out = conv(xd, eid)
    loss = conv.get_attention_loss()
    ref.train(train)
    xr = x.clone().requires_grad_(True)
    want = ref(xr, ei, choices_of(conv, eid, n) if train else None)
    if lin_scale == 1.0:
        assert_no_kink(ref)
    else:
        R.assert_branch_is_sure(ref)
    assert finite(out, loss)
    assert out.shape == want.shape and close(out, want, FWD_TOL), "forward"
    if train:
        print(f"att_loss {loss.item():.6f} vs {ref.att_loss.item():.6f}")
        assert close(loss, ref.att_loss, FWD_TOL), "att_loss"
    else:
        assert loss.item() == 0.0
    cot = R.supergat_cot(ref, n, 1)
    ((out * cot.float().to(dev)).sum() + 4 * loss).backward()
    ((want * cot).sum() + 4 * ref.att_loss).backward()
    grads = {"x": (xd.grad, xr.grad)}
    refp = dict(ref.named_parameters())
    for name, prm in conv.named_parameters():
        grads[name] = (prm.grad, refp[name].grad)
    assert finite(*(a for a, _ in grads.values()))
    for name, (a, b) in grads.items():
        assert close(a, b, GRAD_TOL), name
    return out.detach(), [a for a, _ in grads.values()]


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("graph", R.SUPERGAT_GRAPHS)
@pytest.mark.parametrize("H,C,concat", R.SUPERGAT_SHAPES)
def test_supergat_conv(dev, H, C, concat, graph, train):
    run_supergat(H, C, concat, graph, dev, train)


@pytest.mark.parametrize("train", [False, True])
def test_supergat_conv_with_saturated_sigmoid(dev, train):
    """d = <h_i, h_j> beyond +-30: float32's sigmoid is exactly 1 or vanishes, the link loss's softplus is linear."""
    H, C, concat, graph, lin_scale = R.SUPERGAT_WIDE
    run_supergat(H, C, concat, graph, dev, train, lin_scale=lin_scale)


# ---- masked cross-entropy ---------------------------------------------------------------------------------------------

def run_loss(C, kind, dev):
    """The loss kernels on materialised logits and the loss epilogue of the gather (statistics form, gradient form) against
    float64 log_softmax + NLL of the very logits the device formed (the epilogue's rows are bit-identical to the plain
    gather's). The gradient is that of the SUM of the selected rows' losses (scale 1): -1 / +1 stay -1 / +1."""
    from rgb_experiment_amd import ops
    from test_gpu_rows import _kind_graph
    ei, h, bias, y, mask = R.loss_case(C)
    n, d = R.LOSS_N, (C + 3) // 4 * 4
    g = _kind_graph(dev, ei, n, kind)
    assert g.fwd.split is not None
    h_d, bias_d, y_d, mask_d = h.to(dev), bias.to(dev), y.to(dev), mask.to(dev)
    w, rs = ops._kind_weights(g, kind)
    gather = dict(y=h_d[:, d:], a=1.0, b=1.0, bias=bias_d)
    logits = ops.spmm_raw(g.fwd, w, rs, h_d[:, :d], **gather)[:, :C].contiguous()
    z = logits.cpu()
    R.assert_loss_profile(R.loss_profile(z, y, mask, C), C)
    nll, count, hits, grad = R.loss_reference(z, y, mask, C)

    def check_stats(stats, what):
        stats = stats.cpu()
        assert finite(stats), what
        print(f"{what}: nll {stats[0].item():.4f} vs {nll:.4f}, rows {int(stats[1])} vs {count}, hits {int(stats[2])} vs {hits}")
        assert abs(stats[0].item() - nll) < 1e-5 * max(1.0, abs(nll)), what
        assert int(stats[1].item()) == count and int(stats[2].item()) == hits, what

    def check_grad(got, what):
        got = got.cpu()
        assert finite(got), what
        err = (got.double() - grad).abs().max().item()
        print(f"{what}: max |gradient - ref| {err:.3e}")
        assert err < 1e-6, what
        rows = torch.tensor(list(R.LOSS_SURE_ROWS))
        if C > 1:  # probability 1 on the target: exactly 0; probability 0: -1 on the target
            assert torch.equal(got[rows], torch.zeros(len(rows), C)), what
            lost = torch.tensor(list(R.LOSS_LOST_ROWS))
            assert torch.equal(got[lost, y[lost]], torch.full((len(lost),), -1.0)), what

    check_stats(ops.masked_ce_accuracy(logits, y_d, mask_d), "masked_ce_accuracy")
    lg = logits.clone().requires_grad_(True)
    loss, stats = ops.masked_ce_loss(lg, y_d, mask_d, reduction="sum", with_stats=True)
    check_stats(stats, "masked_ce_loss")
    assert abs(loss.item() - nll) < 1e-5 * max(1.0, abs(nll))
    loss.backward()
    check_grad(lg.grad, "masked_ce_loss")
    mean = ops.masked_ce_loss(logits, y_d, mask_d)
    assert abs(mean.item() - nll / count) < 1e-5 * max(1.0, abs(nll / count))
    none, stats_e = ops.spmm_epilogue_raw(g.fwd, w, rs, h_d[:, :d], ce=(y_d, mask_d, None), n_classes=C, **gather)
    assert none is None
    check_stats(stats_e, "epilogue, statistics form")
    one = torch.ones(1, device=dev)
    grad_e, stats_g = ops.spmm_epilogue_raw(g.fwd, w, rs, h_d[:, :d], ce=(y_d, mask_d, one), n_classes=C, **gather)
    assert torch.equal(stats_g, stats_e)
    check_grad(grad_e[:, :C], "epilogue, gradient form")
    assert torch.equal(grad_e[:, C:], torch.zeros(n, d - C, device=dev))
    return stats_e, grad_e, lg.grad


@pytest.mark.parametrize("kind", ["gcn", "mean"])
@pytest.mark.parametrize("C", R.LOSS_CLASSES)
def test_masked_cross_entropy(dev, C, kind, monkeypatch):
    from rgb_experiment_amd import graph as G
    monkeypatch.setattr(G, "LONG_ROW_SLOTS", 256)  # as test_row_kernel_cross_entropy: the hub row's logits come from chunks
    run_loss(C, kind, dev)


# ---- reproducibility ----------------------------------------------------------------------------------------------------

def same_bits(a, b):
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("family", ["gatv2", "gat", "supergat", "loss"])
def test_two_runs_are_bit_identical(dev, family, monkeypatch):
    """One case per family, hub rows included, twice: same bits (no float atomics, fixed summation orders). SuperGAT in
    eval mode: its training mode adds the negative pairs' row gradients with float atomics."""
    from rgb_experiment_amd import graph as G
    if family == "loss":
        monkeypatch.setattr(G, "LONG_ROW_SLOTS", 256)
        for x, y in zip(run_loss(47, "gcn", dev), run_loss(47, "gcn", dev)):
            assert torch.equal(x, y)
        return
    run = {"gatv2": lambda: run_gatv2(8, 8, "powerlaw", dev, True, torch_seed=21),
           "gat": lambda: run_gat_aggregate(8, 8, "hub", dev),
           "supergat": lambda: run_supergat(8, 8, True, "hub", dev, False)}[family]
    same_bits(run(), run())
