"""TransformerConv on the MI355X: ops.transformer_attend (eval and training mode, every lane layout, hub rows, rows
without in-edges, sources without out-edges, a graph without edges), scores far beyond the range of an unshifted expf,
TransformerConv, the GraphTransformer model and experiment(model_name="transformer") against the float64 restatement of
tests/test_transformer_host.py, which is fed the exact dropout decisions the device made
(ops.transformer_random_choices). The cases are that file's; it checks on the CPU that each is well-posed.

Tolerances are those of tests/test_gpu_gatv2.py for the same depth of fp32 gather: forward 1e-4 * max(1, |ref|max),
gradients 2e-4 * max(1, |ref|max). Every element is compared.

Rows the kernels have no slot for. The op allocates its output, its gradients and the per-node record with torch.empty.
Before every operator call the allocator's free blocks of those sizes are filled with NaN (`poison`), so a row that a
kernel skipped shows as NaN in the comparison instead of passing on stale zeros; `finite` is asserted on top."""
import functools
import math

import numpy as np
import pytest
import torch

import test_transformer_host as T
from test_gpu_ggnn import close, rand_graph

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = T.FWD_TOL, T.GRAD_TOL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def device_graph(ei, n, dev):
    from rgb_experiment_amd.graph import LOOPS_KEEP, get_graph
    return get_graph(ei.to(dev), n, LOOPS_KEEP)


@functools.lru_cache(maxsize=None)
def operator_graph(name, dev):
    """The device graph of a host-file graph, with what the cases rely on asserted once."""
    ei, n = T.graph_of(name)
    graph = device_graph(ei, n, dev)
    assert graph.fwd.nnz == ei.size(1) and graph.bwd.nnz == ei.size(1)        # nothing added, nothing coalesced
    if name == "random":
        indeg = (graph.fwd.rowptr[1:] - graph.fwd.rowptr[:-1]).cpu()
        outdeg = (graph.bwd.rowptr[1:] - graph.bwd.rowptr[:-1]).cpu()
        assert int((indeg == 0).sum()) >= 20 and int((outdeg == 0).sum()) >= 20
        assert int((ei[0] == ei[1]).sum()) > 0                                # self-loops stay
        assert torch.unique(ei[0] * n + ei[1]).numel() < ei.size(1)           # duplicates stay
    if name == "powerlaw":
        assert graph.fwd.split is not None and graph.bwd.split is not None    # both row-split paths run
    if name == "no_edges":
        assert graph.fwd.nnz == 0
    return graph


def choices_of(record, graph, H):
    from rgb_experiment_amd import ops
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in ops.transformer_random_choices(record, graph, H).items()}


POISON_BLOCKS = 12  # per size; the op and autograd allocate at most 6 of the widest (out, out * cot, gout, g_q, g_k, g_v)


def poison(dev, *shapes):
    """Fill POISON_BLOCKS free blocks of each of these sizes with NaN and hand them back to the allocator: twice as many
    as the op and autograd take of any one size, so every torch.empty of such a size gets one of them."""
    blocks = [torch.full(s, float("nan"), dtype=torch.float32, device=dev) for s in shapes for _ in range(POISON_BLOCKS)]
    torch.cuda.synchronize()
    del blocks


def finite(*tensors):
    return all(bool(torch.isfinite(t).all()) for t in tensors)


def run_operator(H, C, graph_name, dev, train, torch_seed=5, large=False):
    """ops.transformer_attend forward and g_q, g_k, g_v against the restatement."""
    from rgb_experiment_amd import ops
    _, n = T.graph_of(graph_name)
    graph = operator_graph(graph_name, dev)
    p = 0.5 if train else 0.0
    case = T.large_case(H, C, graph_name) if large else T.operator_case(H, C, graph_name)
    leaf = lambda t: t.float().to(dev).requires_grad_(True)
    q_d, k_d, v_d = leaf(case[0]), leaf(case[1]), leaf(case[2])
    cot_d = case[3].float().to(dev)
    record = {}
    torch.manual_seed(torch_seed)
    poison(dev, (n, H * C), (n, H), (n, H, 2))
    out = ops.transformer_attend(q_d, k_d, v_d, graph, H, C, 1.0 / math.sqrt(C), training=train, p_drop=p, record=record)
    (out * cot_d).sum().backward()
    assert finite(out, q_d.grad, k_d.grad, v_d.grad), "a row was left unwritten"
    if train:
        ch = choices_of(record, graph, H)
        assert record["seed"] is not None and ch["keep"].shape == (graph.fwd.nnz, H)
        want = T.run_formula(case, graph_name, H, C, src=ch["src"], dst=ch["dst"], keep=ch["keep"], p=p)
    else:
        assert record["seed"] is None
        want = T.eval_reference(H, C, graph_name, large=large)
    assert close(out, want[0], FWD_TOL), "forward"
    assert close(q_d.grad, want[1][0], GRAD_TOL), "g_q"
    assert close(k_d.grad, want[1][1], GRAD_TOL), "g_k"
    assert close(v_d.grad, want[1][2], GRAD_TOL), "g_v"
    if graph_name == "no_edges":  # exact zeros, not small numbers
        for t in (out, q_d.grad, k_d.grad, v_d.grad):
            assert t.abs().max().item() == 0.0
    if graph_name == "random":    # rows without in-edges / sources without out-edges: exact zeros
        assert out[:20].abs().max().item() == 0.0 and q_d.grad[:20].abs().max().item() == 0.0
        assert k_d.grad[20:40].abs().max().item() == 0.0 and v_d.grad[20:40].abs().max().item() == 0.0
    return out.detach(), (q_d.grad, k_d.grad, v_d.grad)


@pytest.mark.parametrize("graph", T.GRAPH_NAMES)
@pytest.mark.parametrize("H,C", T.PAIRS)
def test_attend_eval_forward_backward(dev, H, C, graph):
    from rgb_experiment_amd import ops
    assert ops.transformer_supported(H, C)
    run_operator(H, C, graph, dev, train=False)


@pytest.mark.parametrize("graph", T.GRAPH_NAMES)
@pytest.mark.parametrize("H,C", T.PAIRS)
def test_attend_training_forward_backward(dev, H, C, graph):
    run_operator(H, C, graph, dev, train=True)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("graph", T.LARGE_GRAPHS)
@pytest.mark.parametrize("H,C", T.LARGE_PAIRS)
def test_attend_large_scores(dev, H, C, graph, train):
    """Scores of standard deviation 128 (|e| up to several hundred; late maxima in long rows and hub-row chunks with
    maxima far apart on `powerlaw`: tests/test_transformer_host.py asserts it), at the unchanged tolerances."""
    run_operator(H, C, graph, dev, train=train, large=True)


def test_attend_refusals_and_inference_form(dev):
    from rgb_experiment_amd import ops
    _, n = T.graph_of("random")
    graph = operator_graph("random", dev)
    g = torch.Generator().manual_seed(3)
    wide = lambda w: torch.randn(n, w, generator=g).to(dev)
    assert not ops.transformer_supported(1, 67) and not ops.transformer_supported(1, 130)
    with pytest.raises(RuntimeError, match="pad the head width"):
        ops.transformer_attend(wide(67), wide(67), wide(67), graph, 1, 67, 67 ** -0.5)
    with pytest.raises(ValueError, match="dropout"):
        ops.transformer_attend(wide(8), wide(8), wide(8), graph, 1, 8, 8 ** -0.5, training=True, p_drop=1.0)
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.transformer_attend(wide(16), wide(16), wide(8), graph, 2, 8, 8 ** -0.5)
    # no gradient wanted: the kernel's inference form (m == NULL) stores the same bits, on rows cut into chunks too
    for name in ("random", "powerlaw"):
        graph = operator_graph(name, dev)
        q, k, v = (t.float().to(dev) for t in T.operator_case(2, 8, name)[:3])
        with torch.no_grad():
            plain = ops.transformer_attend(q, k, v, graph, 2, 8, 8 ** -0.5)
        saved = ops.transformer_attend(q.clone().requires_grad_(True), k, v, graph, 2, 8, 8 ** -0.5)
        assert saved.grad_fn is not None and plain.grad_fn is None
        assert torch.equal(plain, saved.detach())


# ---- layer ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", sorted(T.LAYER_CASES))
def test_layer_forward_backward(dev, name, train):
    """Output and the gradients of x and of every parameter; the parameter names are the reference's (PyG's). The padded
    cases would come out wrong with the scale of the padded width: 1 / sqrt(68) against 1 / sqrt(67) moves every score
    by 0.7 %."""
    from rgb_experiment_amd.nn import GATConv, TransformerConv
    H, C, kw = T.LAYER_CASES[name]
    p = 0.5 if train else 0.0
    x, ei, ref = T.layer_case(name, p)
    conv = TransformerConv(T.LAYER_F, C, heads=H, dropout=p, **kw)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    conv.to(dev).train(train)
    ref.train(train)
    assert (GATConv.kernel_channels(C) != C) == name.startswith("padded")
    xd = x.float().to(dev).requires_grad_(True)
    torch.manual_seed(5)
    out = conv(xd, ei.to(dev))
    ch = choices_of(conv.last_draw, device_graph(ei, T.LAYER_N, dev), H) if train else None
    assert (conv.last_draw["seed"] is not None) == train
    xr_ = x.clone().requires_grad_(True)
    want = ref(xr_, ei, ch)
    assert out.shape == want.shape and finite(out) and close(out, want, FWD_TOL), "forward"
    cot = T.f32_exact(want.shape, torch.Generator().manual_seed(17))
    (out * cot.float().to(dev)).sum().backward()
    (want * cot).sum().backward()
    assert close(xd.grad, xr_.grad, GRAD_TOL), "g_x"
    refp = dict(ref.named_parameters())
    got = dict(conv.named_parameters())
    assert sorted(got) == sorted(refp)
    for k, prm in got.items():
        if refp[k].grad is None:  # lin_skip without root_weight: present (PyG's layout) and unused, on both sides
            assert k.startswith("lin_skip") and not conv.root_weight and prm.grad is None
            continue
        assert prm.grad is not None and finite(prm.grad) and close(prm.grad, refp[k].grad, GRAD_TOL), k


@pytest.mark.parametrize("name", ["padded_67", "padded_130"])
def test_scale_under_padding(dev, name):
    """The scale the layer passes is that of the TRUE head width, and the output follows it: against a reference scored
    with the padded width's scale the same output is far outside the tolerance."""
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.nn import GATConv, TransformerConv
    H, C, kw = T.LAYER_CASES[name]
    Cp = GATConv.kernel_channels(C)
    assert Cp != C
    x, ei, ref = T.layer_case(name)
    conv = TransformerConv(T.LAYER_F, C, heads=H, **kw)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    conv.to(dev).eval()
    seen = {}
    attend = ops.transformer_attend

    def spy(q, k, v, graph, H_, C_, scale, **kwargs):
        seen.update(H=H_, C=C_, scale=scale)
        return attend(q, k, v, graph, H_, C_, scale, **kwargs)
    ops.transformer_attend = spy
    try:
        with torch.no_grad():
            out = conv(x.float().to(dev), ei.to(dev))
    finally:
        ops.transformer_attend = attend
    assert seen["C"] == Cp and seen["H"] == H
    assert seen["scale"] == 1.0 / math.sqrt(C) and seen["scale"] != 1.0 / math.sqrt(Cp)
    ref.eval()
    with torch.no_grad():
        want = ref(x, ei)
        n = x.size(0)
        wrong, _ = T.attend(ref.lin_query(x).view(n, H, C), ref.lin_key(x).view(n, H, C), ref.lin_value(x).view(n, H, C),
                            n, ei[0], ei[1], 1.0 / math.sqrt(Cp))
        wrong = wrong.reshape(n, H * C) + ref.lin_skip(x)
    assert close(out, want, FWD_TOL)
    assert (out.cpu().double() - wrong).abs().max().item() > 10 * FWD_TOL * max(1.0, want.abs().max().item())


# ---- model ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(), dict(beta=True)], ids=["plain", "beta"])
def test_model_against_restatement(dev, kw):
    """Logits, `emb` and every parameter gradient of one training step (BatchNorm on batch statistics)."""
    x, y, ei, model, ref = T.model_case(**kw)
    model.to(dev).train()
    ref.train()
    res = model(x.float().to(dev), ei.to(dev))
    want = ref(x, ei)
    assert close(res["emb"], want["emb"], FWD_TOL) and close(res["out"], want["out"], FWD_TOL)
    torch.nn.functional.nll_loss(res["out"], y.to(dev)).backward()
    torch.nn.functional.nll_loss(want["out"], y).backward()
    refp = dict(ref.named_parameters())
    got = dict(model.named_parameters())
    assert sorted(got) == sorted(refp)
    for name, prm in got.items():
        assert prm.grad is not None and close(prm.grad, refp[name].grad, GRAD_TOL), name


# ---- dropout, determinism --------------------------------------------------------------------------------------------

def test_dropout_draws(dev):
    """Kept share within 5 standard deviations of 1 - p, overall and per head; E * H draws (no added loops); one seed twice
    is bit-identical; two seeds differ; p = 0 in training mode equals eval mode bit for bit."""
    from rgb_experiment_amd import ops
    n, E, H, C, p = 5000, 40000, 8, 8, 0.5
    ei = rand_graph(n, E, 17, loops=5, dups=30)
    graph = device_graph(ei, n, dev)
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(n, H * C, generator=g).to(dev) for _ in range(3))

    def run(seed, p_drop=p, training=True):
        rec = {}
        torch.manual_seed(seed)
        out = ops.transformer_attend(q, k, v, graph, H, C, C ** -0.5, training=training, p_drop=p_drop, record=rec)
        return out, rec
    out_a, rec_a = run(5)
    keep_a = choices_of(rec_a, graph, H)["keep"]
    draws = keep_a.numel()
    assert draws == ei.size(1) * H == (E + 5 + 30) * H
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

@pytest.mark.parametrize("beta", [False, True])
def test_experiment_trains_and_hip_graph_equals_eager(dev, beta):
    import rgb_experiment_amd as R
    n, f, c, epochs = 300, 16, 4, 5
    gen = torch.Generator().manual_seed(11)
    ei = rand_graph(n, 1800, 13, loops=4, dups=4)
    data = R.Data(x=torch.randn(n, f, generator=gen), y=torch.randint(0, c, (n,), generator=gen), edge_index=ei)
    params = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0, "heads": 4, "att_dropout": 0.0, "beta": beta}
    runs = []
    for graphed in (False, True):
        runs.append(R.experiment(params, specify_data=True, data=data, model_name="transformer", learning_rate=0.01,
                                 epoch=epochs, need_to_reappear=True, print_print=False, return_model=True,
                                 use_hip_graph=graphed, implement_early_stopping=False))
    a, b = runs
    from rgb_experiment_amd.models import GraphTransformer
    assert isinstance(a["model"], GraphTransformer) and (a["model"].convs[0].lin_beta is not None) == beta
    for key in ("ACC", "precision_score", "recall_score", "f1_macro", "f1_micro"):
        assert key in a and np.isfinite(float(a[key])), key
    assert b["used_hip_graph"] and not a["used_hip_graph"]
    assert len(a["history"]["train_loss"]) == epochs and len(b["history"]["train_loss"]) == epochs
    for key in ("train_loss", "val_loss", "test_loss"):
        assert np.allclose(a["history"][key], b["history"][key], rtol=0, atol=1e-6), key
    for key in ("train_acc", "val_acc", "test_acc"):
        assert a["history"][key] == b["history"][key], key
