"""GATv2 on the MI355X: ops.gatv2_attend (eval and training mode, every lane layout, hub rows, a graph of self-loops
only), GATv2Conv, the GATv2 model and experiment(model_name="gatv2") against the float64 restatement of
tests/test_gatv2_host.py, which is fed the exact dropout decisions the device made (ops.gatv2_random_choices).

Tolerances are those tests/test_gpu_supergat.py and tests/test_gpu_fagcn.py use for the same depth of fp32 gather:
forward 1e-4 * max(1, |ref|max), gradients 2e-4 * max(1, |ref|max). Every element is compared.

LeakyReLU's kink. At the operator level s = xl + xr is ONE fp32 addition of values both sides hold exactly, so its sign
is the float64 sign and the gradient checks are strict by construction. At the layer and model level xl and xr come out
of an fp32 product over K <= 32 inputs of order 1, whose rounding is bounded by (K + 2) * 2^-24 * sum |x_k w_k| < 1e-5:
a pre-activation that close to zero could take the other slope on the device, which moves one gradient element by
O(de * att) — no rounding error. The cases are therefore chosen (seeds scanned on the CPU, reference only) so that the
float64 reference has NO (slot, head, channel) pre-activation below the bound, and each test asserts that count is 0:
|s| < 1e-5 (the rounding bound itself) for the single layers, |s| < 1e-4 in every layer for the model."""
import functools

import numpy as np
import pytest
import torch

from test_gatv2_host import RefGATv2, RefGATv2Conv, rewritten_edges
from test_gpu_fagcn import powerlaw_graph
from test_gpu_ggnn import close, rand_graph

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = 1e-4, 2e-4
SLOPE = 0.2
PAIRS = [(1, 4), (1, 7), (2, 8), (8, 8), (3, 5), (8, 40), (1, 64), (1, 256)]  # (8, 40): heads in several chunks
GRAPH_NAMES = ("empty", "powerlaw", "random")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def graph_of(name):
    """(edge_index, n) of tests/test_gpu_fagcn.py's graphs, built once."""
    if name == "random":
        return rand_graph(700, 6000, 3, loops=11, dups=40), 700
    if name == "powerlaw":
        return powerlaw_graph(), 2000
    return torch.zeros((2, 0), dtype=torch.int64), 50


def device_graph(ei, n, dev):
    from rgb_experiment_amd.graph import LOOPS_REMOVE_ADD, get_graph
    return get_graph(ei.to(dev), n, LOOPS_REMOVE_ADD)


def choices_of(record, graph, H):
    from rgb_experiment_amd import ops
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in ops.gatv2_random_choices(record, graph, H).items()}


def f32_exact(shape, gen, scale=1.0):
    """float64 values that are exactly representable in float32: both sides of a comparison hold the same numbers."""
    return (torch.randn(shape, generator=gen) * scale).double()


def operator_case(H, C, n, seed):
    """xl, xr [n, H*C], att [1, H, C] ~ N(0, 1/C) (scores of order 1), bias [H*C], cotangent: float64, fp32-exact."""
    g = torch.Generator().manual_seed(seed)
    return (f32_exact((n, H * C), g), f32_exact((n, H * C), g), f32_exact((1, H, C), g, C ** -0.5),
            f32_exact((H * C,), g), f32_exact((n, H * C), g))


def run_operator(H, C, graph_name, dev, train, torch_seed=5):
    """ops.gatv2_attend forward and g_xl, g_xr, g_att, g_bias against the restatement."""
    from rgb_experiment_amd import ops
    ei, n = graph_of(graph_name)
    graph = device_graph(ei, n, dev)
    if graph_name == "powerlaw":
        assert graph.fwd.split is not None and graph.bwd.split is not None  # both row-split paths run
    p = 0.5 if train else 0.0
    xl, xr, att, bias, cot = operator_case(H, C, n, 1000 + 10 * H + C)
    leaf = lambda t: t.float().to(dev).requires_grad_(True)
    xl_d, xr_d, att_d, bias_d = leaf(xl), leaf(xr), leaf(att), leaf(bias)
    record = {}
    torch.manual_seed(torch_seed)
    out = ops.gatv2_attend(xl_d, xr_d, att_d, graph, H, C, SLOPE, bias=bias_d, training=train, p_drop=p, record=record)
    (out * cot.float().to(dev)).sum().backward()
    if train:
        ch = choices_of(record, graph, H)
        src, dst, keep = ch["src"], ch["dst"], ch["keep"]
        assert record["seed"] is not None and keep.shape == (src.numel(), H)
    else:
        (src, dst), keep = rewritten_edges(ei, n), None
        assert record["seed"] is None
    ref = RefGATv2Conv(1, C, heads=H, negative_slope=SLOPE, dropout=p)
    xl_r, xr_r, bias_r = (t.clone().requires_grad_(True) for t in (xl, xr, bias))
    with torch.no_grad():
        ref.att.copy_(att)
    want = ref.attend(xl_r.view(n, H, C), xr_r.view(n, H, C), n, src, dst, keep).reshape(n, H * C) + bias_r
    (want * cot).sum().backward()
    assert close(out, want, FWD_TOL), "forward"
    assert close(xl_d.grad, xl_r.grad, GRAD_TOL), "g_xl"
    assert close(xr_d.grad, xr_r.grad, GRAD_TOL), "g_xr"
    assert close(att_d.grad, ref.att.grad, GRAD_TOL), "g_att"
    assert close(bias_d.grad, bias_r.grad, GRAD_TOL), "g_bias"
    return out.detach(), (xl_d.grad, xr_d.grad, att_d.grad)


@pytest.mark.parametrize("graph", GRAPH_NAMES)
@pytest.mark.parametrize("H,C", PAIRS)
def test_attend_eval_forward_backward(dev, H, C, graph):
    from rgb_experiment_amd import ops
    assert ops.gatv2_supported(H, C)
    run_operator(H, C, graph, dev, train=False)


@pytest.mark.parametrize("graph", GRAPH_NAMES)
@pytest.mark.parametrize("H,C", PAIRS)
def test_attend_training_forward_backward(dev, H, C, graph):
    run_operator(H, C, graph, dev, train=True)


def test_attend_refusals_and_inference_form(dev):
    from rgb_experiment_amd import ops
    ei, n = graph_of("random")
    graph = device_graph(ei, n, dev)
    xl, xr, att, bias, _ = operator_case(1, 67, n, 3)
    to = lambda t: t.float().to(dev)
    assert not ops.gatv2_supported(1, 67) and not ops.gatv2_supported(1, 130)
    with pytest.raises(RuntimeError, match="pad the head width"):
        ops.gatv2_attend(to(xl), to(xr), to(att), graph, 1, 67)
    with pytest.raises(ValueError, match="dropout"):
        ops.gatv2_attend(to(xl), to(xr), to(att), graph, 1, 67, training=True, p_drop=1.0)
    # no gradient wanted: the kernel's inference form (m == NULL) stores the same rows
    xl, xr, att, bias, _ = operator_case(2, 8, n, 4)
    with torch.no_grad():
        plain = ops.gatv2_attend(to(xl), to(xr), to(att), graph, 2, 8, bias=to(bias))
    saved = ops.gatv2_attend(to(xl).requires_grad_(True), to(xr), to(att), graph, 2, 8, bias=to(bias))
    assert torch.equal(plain, saved.detach())


# ---- layer ---------------------------------------------------------------------------------------------------------

LAYER_N, LAYER_E, LAYER_F = 120, 500, 12
# name -> (H, C, layer keywords, case seed); the seeds were scanned on the CPU so that the float64 reference has no
# pre-activation with |s| < 1e-5 (see the module docstring); the test asserts it
LAYER_CASES = {
    "unshared": (2, 8, dict(), 0),
    "shared": (2, 8, dict(share_weights=True), 0),
    "mean_of_3_heads": (3, 5, dict(concat=False), 0),
    "no_bias": (2, 8, dict(bias=False), 0),
    "padded_130": (1, 130, dict(), 0),
    "padded_67_shared": (2, 67, dict(share_weights=True), 2),
}
KINK_BOUND_LAYER = 1e-5


def layer_case(name, p=0.0):
    """(x float64 fp32-exact, edge_index, reference layer with every parameter set to fp32-exact random values)."""
    H, C, kw, seed = LAYER_CASES[name]
    g = torch.Generator().manual_seed(7000 + seed)
    ei = rand_graph(LAYER_N, LAYER_E, 7000 + seed, loops=5, dups=12)
    x = f32_exact((LAYER_N, LAYER_F), g)
    ref = RefGATv2Conv(LAYER_F, C, heads=H, negative_slope=SLOPE, dropout=p, **kw)
    with torch.no_grad():
        for name_, prm in ref.named_parameters():
            scale = C ** -0.5 if name_ == "att" else (LAYER_F ** -0.5 if name_.endswith("weight") else 0.5)
            prm.copy_(f32_exact(prm.shape, g, scale))
    return x, ei, ref


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", sorted(LAYER_CASES))
def test_layer_forward_backward(dev, name, train):
    """Output and the gradients of x, lin_l, lin_r, att, bias. With shared weights the one projection's gradient is the
    sum of both roles (the reference shares the module the same way)."""
    from rgb_experiment_amd.nn import GATConv, GATv2Conv
    H, C, kw, _ = LAYER_CASES[name]
    p = 0.5 if train else 0.0
    x, ei, ref = layer_case(name, p)
    conv = GATv2Conv(LAYER_F, C, heads=H, negative_slope=SLOPE, dropout=p, **kw)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    conv.to(dev).train(train)
    ref.train(train)
    assert (GATConv.kernel_channels(C) != C) == name.startswith("padded")
    xd = x.float().to(dev).requires_grad_(True)
    eid = ei.to(dev)
    torch.manual_seed(5)
    out = conv(xd, eid)
    ch = choices_of(conv.last_draw, device_graph(ei, LAYER_N, dev), H) if train else None
    xr_ = x.clone().requires_grad_(True)
    want = ref(xr_, ei, ch)
    near = int((ref.s.abs() < KINK_BOUND_LAYER).sum())
    print(f"{name}: {ref.s.numel()} pre-activations, {near} within {KINK_BOUND_LAYER} of the kink")
    assert near == 0, "the case must keep clear of LeakyReLU's kink: pin another seed"
    assert out.shape == want.shape and close(out, want, FWD_TOL), "forward"
    cot = f32_exact(want.shape, torch.Generator().manual_seed(17))
    (out * cot.float().to(dev)).sum().backward()
    (want * cot).sum().backward()
    assert close(xd.grad, xr_.grad, GRAD_TOL), "g_x"
    refp = dict(ref.named_parameters())
    got = dict(conv.named_parameters())
    assert sorted(got) == sorted(refp)
    for k, prm in got.items():
        assert prm.grad is not None and close(prm.grad, refp[k].grad, GRAD_TOL), k


# ---- model ---------------------------------------------------------------------------------------------------------

MODEL_SEED = 1  # scanned on the CPU: no |s| < 1e-4 in any layer of the float64 reference
MODEL_SHAPE = dict(n=60, e=240, f=16, hidden=4, heads=2, classes=5, layers=3)
KINK_BOUND_MODEL = 1e-4


def model_case(seed):
    from rgb_experiment_amd.models import GATv2
    s = MODEL_SHAPE
    g = torch.Generator().manual_seed(9000 + seed)
    ei = rand_graph(s["n"], s["e"], 9000 + seed, loops=3, dups=6)
    x = f32_exact((s["n"], s["f"]), g)
    y = torch.randint(0, s["classes"], (s["n"],), generator=g)
    torch.manual_seed(9000 + seed)
    model = GATv2(s["layers"], s["hidden"], s["f"], s["classes"], 0.0, s["heads"])
    with torch.no_grad():  # biases off zero, so that their paths are exercised
        for k, prm in model.named_parameters():
            if k.endswith("bias"):
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.3)
    ref = RefGATv2(s["layers"], s["hidden"], s["f"], s["classes"], s["heads"])
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()},
                        strict=True)
    return x, y, ei, model, ref


def test_model_against_restatement(dev):
    """Logits and every parameter gradient of one training step (BatchNorm on batch statistics)."""
    x, y, ei, model, ref = model_case(MODEL_SEED)
    model.to(dev).train()
    ref.train()
    res = model(x.float().to(dev), ei.to(dev))
    want = ref(x, ei)
    near = ref.near_kink(KINK_BOUND_MODEL)
    print(f"pre-activations per layer {[c.s.numel() for c in ref.convs]}, within {KINK_BOUND_MODEL} of the kink: {near}")
    assert sum(near) == 0, "the case must keep clear of LeakyReLU's kink: pin another seed"
    assert close(res["emb"], want["emb"], FWD_TOL) and close(res["out"], want["out"], FWD_TOL)
    torch.nn.functional.nll_loss(res["out"], y.to(dev)).backward()
    torch.nn.functional.nll_loss(want["out"], y).backward()
    refp = dict(ref.named_parameters())
    for name, prm in model.named_parameters():
        assert prm.grad is not None and close(prm.grad, refp[name].grad, GRAD_TOL), name


# ---- dropout, determinism --------------------------------------------------------------------------------------------

def test_dropout_draws(dev):
    """Kept share within 5 standard deviations of 1 - p; one seed twice is bit-identical; two seeds differ; p = 0 in
    training mode equals eval mode bit for bit."""
    from rgb_experiment_amd import ops
    n, H, C, p = 5000, 8, 8, 0.5
    ei = rand_graph(n, 40000, 17, loops=5, dups=30)
    graph = device_graph(ei, n, dev)
    xl, xr, att, bias, _ = operator_case(H, C, n, 2)
    to = lambda t: t.float().to(dev)
    xl, xr, att, bias = to(xl), to(xr), to(att), to(bias)

    def run(seed, p_drop=p, training=True):
        rec = {}
        torch.manual_seed(seed)
        out = ops.gatv2_attend(xl, xr, att, graph, H, C, SLOPE, bias=bias, training=training, p_drop=p_drop, record=rec)
        return out, rec
    out_a, rec_a = run(5)
    keep_a = choices_of(rec_a, graph, H)["keep"]
    draws = keep_a.numel()
    assert draws == (int((ei[0] != ei[1]).sum()) + n) * H
    kept = int(keep_a.sum())
    print(f"kept {kept} of {draws} (slot, head) draws")
    assert abs(kept - (1 - p) * draws) <= 5 * (draws * p * (1 - p)) ** 0.5, kept
    per_head = keep_a.float().mean(0)
    assert bool(((per_head - (1 - p)).abs() < 5 * (p * (1 - p) / keep_a.size(0)) ** 0.5).all()), per_head
    out_b, rec_b = run(5)
    assert torch.equal(out_a, out_b) and torch.equal(keep_a, choices_of(rec_b, graph, H)["keep"])
    out_c, rec_c = run(6)
    assert not torch.equal(keep_a, choices_of(rec_c, graph, H)["keep"]) and not torch.equal(out_a, out_c)
    out_e, rec_e = run(5, training=False)
    out_0, rec_0 = run(5, p_drop=0.0)
    assert rec_e["seed"] is None and rec_0["seed"] is None and torch.equal(out_e, out_0)
    assert bool(choices_of(rec_0, graph, H)["keep"].all())
    assert not torch.equal(out_a, out_e)


@pytest.mark.parametrize("train", [False, True])
def test_two_runs_are_bit_identical(dev, train):
    """No float atomics and fixed summation orders: forward and backward twice on the hub-row graph, same bits."""
    runs = [run_operator(8, 8, "powerlaw", dev, train=train, torch_seed=21) for _ in range(2)]
    (out_a, grads_a), (out_b, grads_b) = runs
    assert torch.equal(out_a, out_b)
    for a, b in zip(grads_a, grads_b):
        assert torch.equal(a, b)


# ---- experiment() ------------------------------------------------------------------------------------------------------

def test_experiment_trains_and_hip_graph_equals_eager(dev):
    import rgb_experiment_amd as R
    n, f, c, epochs = 300, 16, 4, 5
    gen = torch.Generator().manual_seed(11)
    ei = rand_graph(n, 1800, 13, loops=4, dups=4)
    data = R.Data(x=torch.randn(n, f, generator=gen), y=torch.randint(0, c, (n,), generator=gen), edge_index=ei)
    params = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0, "heads": 4, "att_dropout": 0.0}
    runs = []
    for graphed in (False, True):
        runs.append(R.experiment(params, specify_data=True, data=data, model_name="gatv2", learning_rate=0.01,
                                 epoch=epochs, need_to_reappear=True, print_print=False, return_model=True,
                                 use_hip_graph=graphed, implement_early_stopping=False))
    a, b = runs
    from rgb_experiment_amd.models import GATv2
    assert isinstance(a["model"], GATv2)
    for key in ("ACC", "precision_score", "recall_score", "f1_macro", "f1_micro"):
        assert key in a and np.isfinite(float(a[key])), key
    assert b["used_hip_graph"] and not a["used_hip_graph"]
    assert len(a["history"]["train_loss"]) == epochs and len(b["history"]["train_loss"]) == epochs
    for key in ("train_loss", "val_loss", "test_loss"):
        assert np.allclose(a["history"][key], b["history"][key], rtol=0, atol=1e-6), key
    for key in ("train_acc", "val_acc", "test_acc"):
        assert a["history"][key] == b["history"][key], key
