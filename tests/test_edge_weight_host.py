"""Edge weights on the host: the C ABI of the new entry points (argument checks before any launch), header / EXPORTS
agreement, the `edge_weight` keyword of the layers, models and experiment(), and every refusal. No GPU needed."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRIES = ("rgbx_loop_weights_f32", "rgbx_edge_slot_weights_f32", "rgbx_weighted_deg_inv_sqrt_f32",
               "rgbx_gcn_norm_weighted_f32", "rgbx_edge_dot_supported", "rgbx_edge_dot_f32", "rgbx_gcn_norm_bwd_f32")


@pytest.fixture(scope="module")
def lib():
    from rgb_experiment_amd import _lib
    return _lib.load()


def test_header_and_exports_agree_and_version_is_501(lib):
    from rgb_experiment_amd import _lib
    header = open(os.path.join(ROOT, "include", "rgbx_hip.h")).read()
    declared = set(re.findall(r"\b(rgbx_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.EXPORTS)
    for name in NEW_ENTRIES:
        assert name in declared and hasattr(lib, name)
    assert lib.rgbx_version() == 501
    assert "dagnn.py:12-31" in header[header.index("rgbx_loop_weights_f32("):]


def test_new_entries_reject_null_pointers_and_negative_sizes(lib):
    p = 4096  # a non-null, 16-byte aligned fake pointer: every call below must fail BEFORE anything is launched
    assert lib.rgbx_loop_weights_f32(0, p, p, 5, 5, 1, 1.0, p, p, None) == -1
    assert lib.rgbx_loop_weights_f32(p, p, p, -1, 5, 1, 1.0, p, p, None) == -1
    assert lib.rgbx_loop_weights_f32(p, p, p, 5, -1, 1, 1.0, p, p, None) == -1
    assert lib.rgbx_loop_weights_f32(p, p, p, 5, 5, 1, 1.0, 0, p, None) == -1
    assert lib.rgbx_loop_weights_f32(p, p, p, 5, 5, 1, 1.0, p, 0, None) == -1
    assert lib.rgbx_loop_weights_f32(p, p, p, 5, 5, 0, 1.0, p, p, None) == -1  # LOOPS_KEEP adds no loops
    assert lib.rgbx_edge_slot_weights_f32(0, 5, p, 5, p, p, None) == -1
    assert lib.rgbx_edge_slot_weights_f32(p, -1, p, 5, p, p, None) == -1
    assert lib.rgbx_edge_slot_weights_f32(p, 5, p, 5, p, 0, None) == -1
    assert lib.rgbx_edge_slot_weights_f32(p, 9, p, 5, 0, p, None) == -1  # more slots than edges: loop weights needed
    assert lib.rgbx_weighted_deg_inv_sqrt_f32(0, p, 5, p, None) == -1
    assert lib.rgbx_weighted_deg_inv_sqrt_f32(p, 0, 5, p, None) == -1
    assert lib.rgbx_weighted_deg_inv_sqrt_f32(p, p, -1, p, None) == -1
    assert lib.rgbx_weighted_deg_inv_sqrt_f32(p, p, 5, 0, None) == -1
    assert lib.rgbx_gcn_norm_weighted_f32(p, p, 0, 5, p, p, None) == -1
    assert lib.rgbx_gcn_norm_weighted_f32(p, p, p, -1, p, p, None) == -1
    assert lib.rgbx_gcn_norm_weighted_f32(p, p, p, 5, p, 0, None) == -1
    dot = lambda **k: lib.rgbx_edge_dot_f32(k.get("rowptr", p), p, k.get("a", p), k.get("lda", 8), p, 8, k.get("g", p),
                                            k.get("N", 5), k.get("d", 8), None, None)
    assert dot(rowptr=0) == -1 and dot(a=0) == -1 and dot(g=0) == -1 and dot(N=-1) == -1 and dot(d=-4) == -1
    assert dot(lda=4) == -1          # leading dimension < d
    assert dot(d=6) == -5 and dot(d=260) == -5  # RGBX_E_SHAPE: pad / cut the rows
    assert dot(a=p + 4) == -3        # RGBX_E_ALIGN
    assert lib.rgbx_edge_dot_supported(128) == 1 and lib.rgbx_edge_dot_supported(7) == 0
    bwd = lambda **k: lib.rgbx_gcn_norm_bwd_f32(k.get("rowptr", p), p, p, p, p, k.get("t2f", p), p, k.get("g", p), p, p,
                                                k.get("N", 5), k.get("E", 5), p, k.get("dew", p), None)
    assert bwd(rowptr=0) == -1 and bwd(t2f=0) == -1 and bwd(g=0) == -1 and bwd(N=-1) == -1 and bwd(E=-1) == -1
    assert bwd(dew=0) == -1
    assert b"null" in lib.rgbx_last_error_string()


def _toy():
    x = torch.randn(6, 4)
    ei = torch.tensor([[0, 1, 2, 3, 3], [1, 2, 3, 4, 3]])
    return x, ei, torch.rand(5) + 0.5


def test_layers_take_the_keyword_and_refuse_cpu_tensors_with_the_no_fallback_error():
    from rgb_experiment_amd.nn import APPNP, CorrectAndSmooth, GCNConv, SGConv
    from rgb_experiment_amd.nn.correct_and_smooth import LabelPropagation
    x, ei, ew = _toy()
    for layer in (GCNConv(4, 3), APPNP(2, 0.1), SGConv(4, 3, K=2)):
        assert list(inspect.signature(layer.forward).parameters)[:3] == ["x", "edge_index", "edge_weight"]
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            layer(x, ei, ew)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            layer(x, ei, edge_weight=ew)
    conv = GCNConv(4, 3)
    for name in ("forward_folded", "forward_after_bn", "aggregate_input", "_ce"):
        assert "edge_weight" in inspect.signature(getattr(conv, name)).parameters, name
    assert list(inspect.signature(LabelPropagation.__call__).parameters)[1:4] == ["y", "edge_index", "edge_weight"]
    cs = CorrectAndSmooth(2, 0.5, 2, 0.5)
    y_soft = torch.full((6, 3), 1 / 3)
    mask = torch.tensor([True, True, False, False, False, False])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cs.correct(y_soft, torch.tensor([0, 1]), mask, ei, ew)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cs.smooth(y_soft, torch.tensor([0, 1]), mask, ei, edge_weight=ew)


def test_models_take_the_keyword():
    from rgb_experiment_amd.models import GCN, SGC, APPNPStack
    from rgb_experiment_amd.models import GraphSAGE
    x, ei, ew = _toy()
    nets = (GCN(num_layers=2, hidden_unit=8, input_dim=4, output_dim=3, dropout_rate=0.5),
            APPNPStack(hidden_unit=8, input_dim=4, output_dim=3, K=2, alpha=0.1, dropout_rate=0.5),
            SGC(input_dim=4, output_dim=3, K=2))
    for net in nets:
        assert list(inspect.signature(net.forward).parameters) == ["x", "edge_index", "edge_weight"]
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            net(x, ei, edge_weight=ew)
    sage = GraphSAGE(num_layers=2, hidden_unit=8, input_dim=4, output_dim=3, dropout_rate=0.5)
    with pytest.raises(ValueError, match="GCNConv only"):
        sage(x, ei, edge_weight=ew)


def test_weight_contract_is_checked_before_any_launch():
    from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, check_edge_weight, get_graph
    from rgb_experiment_amd.nn import GCNConv
    x, ei, ew = _toy()
    with pytest.raises(ValueError, match="float32"):
        check_edge_weight(ew.double(), ei)
    with pytest.raises(ValueError, match="shape"):
        check_edge_weight(ew[:4], ei)
    with pytest.raises(ValueError, match="shape"):
        check_edge_weight(ew.view(5, 1), ei)
    with pytest.raises(ValueError, match="is on"):
        check_edge_weight(ew.to("meta"), ei)
    for bad in (ew.double(), ew[:3]):  # through the public entry points: ValueError, not the device error behind it
        with pytest.raises(ValueError):
            get_graph(ei, 6, LOOPS_ADD_REMAINING, bad)
        with pytest.raises(ValueError):
            GCNConv(4, 3)(x, ei, bad)


def test_non_finite_weights_are_refused_by_the_weighted_graph():
    """The finiteness check sits in WeightedGraph.__init__ after the contract and the device check; here it is reached
    with a stand-in base graph (no device, no launch)."""
    from rgb_experiment_amd import _lib, graph
    x, ei, ew = _toy()

    class Base:
        N, E, loops_mode, _src, _dst, fwd, _keepalive = 6, 5, 1, ei[0], ei[1], None, ei

    real = _lib.require_device
    _lib.require_device = lambda *t: None
    try:
        for bad in (float("nan"), float("inf")):
            w = ew.clone()
            w[2] = bad
            with pytest.raises(ValueError, match="non-finite"):
                graph.WeightedGraph(Base, w)
        graph.WeightedGraph(Base, ew)  # finite weights pass
    finally:
        _lib.require_device = real


def test_weight_that_requires_grad_is_refused_outside_gcnconv():
    from rgb_experiment_amd.models import SGC, APPNPStack
    from rgb_experiment_amd.nn import APPNP, CorrectAndSmooth, SGConv
    x, ei, ew = _toy()
    ew.requires_grad_(True)
    with pytest.raises(ValueError, match="require grad"):
        APPNP(2, 0.1)(x, ei, ew)
    with pytest.raises(ValueError, match="require grad"):
        SGConv(4, 3, K=2)(x, ei, ew)
    with pytest.raises(ValueError, match="require grad"):
        APPNPStack(hidden_unit=8, input_dim=4, output_dim=3, K=2, alpha=0.1, dropout_rate=0.5)(x, ei, ew)
    with pytest.raises(ValueError, match="require grad"):
        SGC(input_dim=4, output_dim=3, K=2)(x, ei, ew)
    cs = CorrectAndSmooth(2, 0.5, 2, 0.5)
    with pytest.raises(ValueError, match="require grad"):
        cs.smooth(torch.full((6, 3), 1 / 3), torch.tensor([0, 1]),
                  torch.tensor([True, True, False, False, False, False]), ei, ew)


def _data(with_weight):
    from rgb_experiment_amd.data import Data
    g = torch.Generator().manual_seed(5)
    n = 60
    extra = {"edge_weight": torch.rand(300, generator=torch.Generator().manual_seed(6)) + 0.25} if with_weight else {}
    return Data(x=torch.randn(n, 8, generator=g), y=torch.randint(0, 3, (n,), generator=g),
                edge_index=torch.randint(0, n, (2, 300), generator=g), **extra)


def _run(data, **kw):
    from rgb_experiment_amd import experiment
    args = dict(specify_data=True, data=data, remake_data_mask=True, epoch=4, print_print=False, return_model=True,
                need_to_reappear=True, use_cpu=True, model_name="mlp")
    args.update(kw)
    init = args.pop("init", {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.5})
    return experiment(init, **args)


def test_experiment_refusals():
    sig = inspect.signature(__import__("rgb_experiment_amd").experiment).parameters
    assert sig["use_edge_weight"].default is False
    for name in ("mlp", "graphsage", "gat", "gin", "dagnn"):
        with pytest.raises(ValueError, match="gcn, appnpstack, sgc and post_cs"):
            _run(_data(True), model_name=name, use_edge_weight=True)
    with pytest.raises(ValueError, match="to_undirected"):
        _run(_data(True), model_name="gcn", use_edge_weight=True, to_undirected_graph=True)
    with pytest.raises(NotImplementedError, match="partitioned"):
        _run(_data(True), model_name="gcn", use_edge_weight=True, distributed=True)
    with pytest.raises(NotImplementedError):  # the name checks stay in front
        _run(_data(True), model_name="fagcn", use_edge_weight=True)
    with pytest.raises(NotImplementedError):
        _run(_data(True), model_name="gcn", use_edge_weight=True, print_pics=True)


def test_an_unused_edge_weight_attribute_changes_nothing():
    a = _run(_data(False))
    b = _run(_data(True))
    assert a["history"] == b["history"]
    assert a["ACC"] == b["ACC"]
