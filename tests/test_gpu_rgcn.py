"""RGCNConv on the MI355X: the typed view of a graph (slot relations, the mean weights of rgbx_rgcn_slot_norm_f32 bit for
bit, the grouping by relation), ops.rgcn_aggregate in its mix form (every vector width and group count of the lane
layout, head counts in one and in several chunks, hub rows in both CSRs, rows of exactly 0 / 1 / 64 / 65 / T / T + 1
slots, a graph without edges, graphs of one to three nodes, the planted cases) and in its select form, selective backward
passes, strided and offset operands, RGCNConv, the RGCN model and experiment(model_name="rgcn", use_edge_type=True),
against the float64 restatement of tests/test_rgcn_host.py. The cases are that file's; it checks on the CPU that each is
well-posed.

Tolerances are the project's: forward 1e-4 * max(1, |ref|max), gradients 2e-4 * max(1, |ref|max). Every element is
compared. Before every operator call the allocator's free blocks of the sizes the op allocates are filled with NaN
(`poison`), so a row or a slot that a kernel skipped shows as NaN instead of passing on stale zeros; `finite` is asserted
on top."""
import functools

import numpy as np
import pytest
import torch

import test_rgcn_host as H
import test_transformer_host as T
from test_gpu_ggnn import close, rand_graph
from test_gpu_transformer import device_graph, finite, poison
from test_rgcn_host import RGCN, RGCNConv

pytestmark = pytest.mark.gpu

FWD_TOL, GRAD_TOL = T.FWD_TOL, T.GRAD_TOL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def operator_graph(name, dev):
    """The device graph of a host-file graph, with what the cases rely on asserted once."""
    ei, n = H.graph_of(name)
    graph = device_graph(ei, n, dev)
    assert graph.fwd.nnz == ei.size(1) and graph.bwd.nnz == ei.size(1)        # nothing added, nothing coalesced
    if ei.size(1):   # slot p of the device's CSR is edge order[p] of the host file
        assert torch.equal(graph.fwd.perm[:graph.fwd.nnz].cpu().long(), H.slots_of(name)[3])
    if name == "powerlaw":
        assert graph.fwd.split is not None and graph.bwd.split is not None    # both chunk paths run
    if name == "degrees":   # exactly one row beyond the threshold in each CSR: T stays whole, T + 1 is split
        indeg = (graph.fwd.rowptr[1:] - graph.fwd.rowptr[:-1]).cpu()
        outdeg = (graph.bwd.rowptr[1:] - graph.bwd.rowptr[:-1]).cpu()
        assert tuple(indeg[:6].tolist()) == H.G.DEGREES and tuple(outdeg[6:12].tolist()) == H.G.DEGREES
        assert graph.fwd.split["n_long"] == 1 and graph.bwd.split["n_long"] == 1
    return graph


@functools.lru_cache(maxsize=None)
def device_types(name, R, dev):
    """The host file's edge types on the device: ONE tensor per (graph, R), so the typed view is built once."""
    return H.edge_type_of(name, R).to(dev)


def relations_of(name):
    return (H.PLANTED_R,) if name == "planted" else H.RELATIONS


# ---- the typed view --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", H.graph_names + ("planted",))
def test_typed_view(dev, name):
    """etype per slot, w_f = 1.0 / cnt.float() bit for bit, w_t = w_f[t2f], the stable grouping by relation; cached."""
    from rgb_experiment_amd import ops
    graph = operator_graph(name, dev)
    E = graph.E
    for R in relations_of(name):
        et = device_types(name, R, dev)
        poison(dev, (max(E, 1),))
        view = ops.typed_view(graph, et, R)
        assert ops.typed_view(graph, et, R) is view
        assert view.rel.N == R and view.rel.nnz == E and view.rel.rowptr.dtype == torch.int32
        if E == 0:
            assert view.rel.rowptr.abs().max().item() == 0
            continue
        etype, cnt = H.slot_counts(name, R)
        t2f = graph.t2f.long()
        assert view.etype_f.dtype == torch.int32 and torch.equal(view.etype_f.cpu().long(), etype)
        assert torch.equal(view.etype_t, view.etype_f[t2f])
        assert view.w_f.dtype == torch.float32 and finite(view.w_f)
        assert torch.equal(view.w_f.cpu(), 1.0 / cnt.float()), "w_f bits"
        assert torch.equal(view.w_t, view.w_f[t2f])
        assert torch.equal(view.rel.rowptr.cpu().long()[1:], torch.cumsum(torch.bincount(etype, minlength=R), 0))
        assert torch.equal(view.rel.col.cpu().long(), torch.argsort(etype, stable=True))
        if name == "powerlaw":   # a relation holds about E / R slots: a hub row of the grouping
            assert view.rel.split is not None and view.rel.split["n_long"] == max(R - 1, 1)
    assert len(graph.__dict__["_typed_views"]) <= 4


def test_slot_norm_counts_a_hub_row_with_and_without_the_plan(dev):
    """The row of T + 1 slots counted by its two chunk waves (the plan) and by one wave (no plan): the same bits."""
    import ctypes
    from rgb_experiment_amd import _lib, ops
    graph = operator_graph("degrees", dev)
    view = ops.typed_view(graph, device_types("degrees", 3, dev), 3)
    poison(dev, (graph.E,))
    w = torch.empty(graph.E, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().rgbx_rgcn_slot_norm_f32(_lib.ptr(graph.fwd.rowptr), _lib.ptr(view.etype_f), _lib.ptr(w), graph.N,
                                                   3, None, _lib.stream_ptr()), "rgbx_rgcn_slot_norm_f32")
    assert torch.equal(w, view.w_f)


def test_typed_view_refusals_and_rebuild(dev):
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_REMOVE_ADD, get_graph
    graph = operator_graph("random", dev)
    _, n = H.graph_of("random")
    et = H.edge_type_of("random", 3).to(dev)                              # a tensor of its own: it is edited below
    with pytest.raises(ValueError, match="outside"):
        ops.typed_view(graph, et, 1)                                      # the values reach 1
    with pytest.raises(ValueError, match="outside"):
        ops.typed_view(graph, et - 1, 3)
    with pytest.raises(RuntimeError, match="LOOPS_KEEP"):
        ops.typed_view(get_graph(graph._keepalive, n, LOOPS_REMOVE_ADD), et, 3)
    a = ops.typed_view(graph, et, 3)
    et.copy_((et + 1) % 3)                                                # in place: the version moves, the view is rebuilt
    b = ops.typed_view(graph, et, 3)
    assert b is not a and torch.equal(b.etype_f, (a.etype_f + 1) % 3)
    assert ops.typed_view(graph, et, 4) is not b                          # R is part of the key


# ---- the mix form ------------------------------------------------------------------------------------------------------

def run_mix(B, C, R, graph_name, aggr, dev, needs=(True, True, True), sink=None):
    """ops.rgcn_aggregate with comp: forward and the gradients asked for (`needs`: of h, comp, y0)."""
    from rgb_experiment_amd import ops
    ei, n = H.graph_of(graph_name)
    graph = operator_graph(graph_name, dev)
    h, comp, y0, cot = (t.float().to(dev) for t in H.mix_case(B, C, R, graph_name))
    h, comp, y0 = (t.requires_grad_(need) for t, need in zip((h, comp, y0), needs))
    et = device_types(graph_name, R, dev)
    ops.typed_view(graph, et, R)                                          # built before the poison, as in a second step
    poison(dev, (n, C), (n, B * C), (max(ei.size(1), 1), B), (R, B))
    if sink is not None:
        ops.set_event_sink(sink)
    try:
        out = ops.rgcn_aggregate(h, graph, et, R, comp=comp, aggr=aggr, y0=y0)
        if any(needs):
            (out * cot).sum().backward()
    finally:
        ops.set_event_sink(None)
    return out.detach(), [h.grad, comp.grad, y0.grad]


def check_mix(B, C, R, graph_name, aggr, dev):
    out, grads = run_mix(B, C, R, graph_name, aggr, dev)
    assert finite(out, *grads), "a row or a slot was left unwritten"
    want = H.mix_reference(B, C, R, graph_name, aggr)
    assert close(out, want[0], FWD_TOL), "forward"
    for name, got, ref in zip(H.MIX_NAMES[1:], grads, want[1]):
        assert got.shape == ref.shape and close(got, ref, GRAD_TOL), name
    y0 = H.mix_case(B, C, R, graph_name)[2].float()
    if R > 1 and graph_name != "planted":
        assert grads[1][R - 1].abs().max().item() == 0.0, "g_comp of the relation without an edge"
    if graph_name == "no_edges":
        assert torch.equal(out.cpu(), y0) and grads[0].abs().max().item() == 0.0 and grads[1].abs().max().item() == 0.0
    if graph_name == "random":            # rows without in-edges store y0; sources without out-edges get zeros
        assert torch.equal(out[:20].cpu(), y0[:20]) and grads[0][20:40].abs().max().item() == 0.0
    assert torch.equal(grads[2].cpu(), H.mix_case(B, C, R, graph_name)[3].float())   # g_y0 is the cotangent
    return out, grads


@pytest.mark.parametrize("B,C,R,graph,aggr", H.MIX_CASES)
def test_mix_forward_backward(dev, B, C, R, graph, aggr):
    from rgb_experiment_amd import ops
    assert ops.rgcn_mix_supported(B, C)
    check_mix(B, C, R, graph, aggr, dev)


def test_mix_cases_cover_the_layout():
    vec = lambda C: 4 if C % 4 == 0 else (2 if C % 2 == 0 else 1)
    for graph in ("degrees", "powerlaw"):
        assert {vec(C) for _, C, _, g, _ in H.MIX_CASES if g == graph} == {1, 2, 4}
        assert {R for _, _, R, g, _ in H.MIX_CASES if g == graph} == set(H.RELATIONS)
    assert {(B, C) for B, C, _, g, _ in H.MIX_CASES if g == "degrees"} >= set(H.MIX_PAIRS)


def test_mix_without_y0_stores_zeros_in_empty_rows(dev):
    from rgb_experiment_amd import ops
    graph = operator_graph("random", dev)
    h, comp, y0, _ = (t.float().to(dev) for t in H.mix_case(2, 7, 3, "random"))
    et = device_types("random", 3, dev)
    _, n = H.graph_of("random")
    poison(dev, (n, 7))
    with torch.no_grad():
        bare = ops.rgcn_aggregate(h, graph, et, 3, comp=comp)
        full = ops.rgcn_aggregate(h, graph, et, 3, comp=comp, y0=y0)
    assert finite(bare) and bare[:20].abs().max().item() == 0.0
    assert close(full - bare, y0.cpu().double(), FWD_TOL)


@pytest.mark.parametrize("graph", ["random", "powerlaw"])
def test_selective_passes(dev, graph):
    """Only h asks for a gradient: only the source pass is launched; only comp: only the coefficient pass and its
    reduction; y0 alone: neither. What is computed has the bits of the full backward."""
    B, C, R = 5, 16, 3
    _, full = run_mix(B, C, R, graph, "mean", dev)
    for needs, launched in (((True, False, False), ["rgcn_mix_fwd", "rgcn_mix_bwd_src"]),
                            ((False, True, False), ["rgcn_mix_fwd", "rgcn_mix_bwd_coef", "rgcn_comp_reduce"]),
                            ((False, False, True), ["rgcn_mix_fwd"]),
                            ((False, False, False), ["rgcn_mix_fwd"]),
                            ((True, True, True), ["rgcn_mix_fwd", "rgcn_mix_bwd_src", "rgcn_mix_bwd_coef",
                                                  "rgcn_comp_reduce"])):
        sink = []
        _, got = run_mix(B, C, R, graph, "mean", dev, needs=needs, sink=sink)
        torch.cuda.synchronize()
        assert [str(kind) for kind, _, _ in sink if str(kind).startswith("rgcn")] == launched
        for need, a, b in zip(needs, got, full):
            assert (a is None) == (not need) and (a is None or torch.equal(a, b))


def test_two_runs_are_bit_identical(dev):
    """No float atomics and fixed summation orders: forward and backward twice on the hub-row graph, same bits."""
    for B, C in ((8, 64), (30, 16)):
        (out_a, grads_a), (out_b, grads_b) = [run_mix(B, C, 7, "powerlaw", "mean", dev) for _ in range(2)]
        assert torch.equal(out_a, out_b) and all(torch.equal(a, b) for a, b in zip(grads_a, grads_b))


def test_strided_and_offset_operands(dev):
    """h and y0 as column blocks of wider matrices and a column-major cotangent give the bits of contiguous operands; an
    h that starts off the 16-byte grid is read one float at a time (another order of the sums: the tolerances)."""
    from rgb_experiment_amd import ops
    B, C, R = 2, 64, 3
    graph = operator_graph("random", dev)
    et = device_types("random", R, dev)
    h, comp, y0, cot = (t.float().to(dev) for t in H.mix_case(B, C, R, "random"))
    F = B * C

    def run(hv, yv, cotv, wide):
        hv, yv, cv = hv.detach().requires_grad_(True), yv.detach().requires_grad_(True), comp.detach().requires_grad_(True)
        hs, ys = (hv[:, 8:8 + F], yv[:, 4:4 + C]) if wide else (hv, yv)
        out = ops.rgcn_aggregate(hs, graph, et, R, comp=cv, y0=ys)
        (out * cotv).sum().backward()
        return out.detach(), ((hv.grad[:, 8:8 + F], yv.grad[:, 4:4 + C]) if wide else (hv.grad, yv.grad)) + (cv.grad,)

    plain_out, plain_grads = run(h, y0, cot, False)
    pad = torch.nn.functional.pad
    wide_out, wide_grads = run(pad(h, (8, 8)), pad(y0, (4, 12)), cot.t().contiguous().t(), True)
    assert torch.equal(plain_out, wide_out)
    assert all(torch.equal(a, b) for a, b in zip(plain_grads, wide_grads))
    flat = torch.zeros(h.numel() + 1, device=dev)
    flat[1:] = h.reshape(-1)
    off_grid = flat[1:].view_as(h)
    assert off_grid.data_ptr() % 16 == 4
    off_out, off_grads = run(off_grid, y0, cot, False)
    assert close(off_out, plain_out.cpu().double(), FWD_TOL)
    assert all(close(a, b.cpu().double(), GRAD_TOL) for a, b in zip(off_grads, plain_grads))


def test_comp_is_read_on_the_device(dev):
    """comp changed in place between two forwards changes the output: nothing of it is cached on the host."""
    from rgb_experiment_amd import ops
    B, C, R = 2, 7, 3
    graph = operator_graph("random", dev)
    et = device_types("random", R, dev)
    case = H.mix_case(B, C, R, "random")
    h, comp, y0, _ = (t.float().to(dev) for t in case)
    with torch.no_grad():
        a = ops.rgcn_aggregate(h, graph, et, R, comp=comp, y0=y0)
        comp.mul_(2.0)
        b = ops.rgcn_aggregate(h, graph, et, R, comp=comp, y0=y0)
    assert not torch.equal(a, b)
    doubled = (case[0], 2 * case[1], case[2], case[3])
    assert close(b, H.run_mix(doubled, R, "random", "mean")[0], FWD_TOL)


def test_mix_refusals(dev):
    from rgb_experiment_amd import ops
    graph = operator_graph("random", dev)
    _, n = H.graph_of("random")
    et = device_types("random", 3, dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    assert not ops.rgcn_mix_supported(2, 67) and not ops.rgcn_mix_supported(65, 8)
    with pytest.raises(RuntimeError, match="pad the width"):
        ops.rgcn_aggregate(z(n, 2 * 67), graph, et, 3, comp=z(3, 2))
    with pytest.raises(RuntimeError, match="1 <= B <= 64"):
        ops.rgcn_aggregate(z(n, 65 * 4), graph, et, 3, comp=z(3, 65))
    with pytest.raises(RuntimeError, match="comp"):
        ops.rgcn_aggregate(z(n, 8), graph, et, 3, comp=z(4, 2))
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.rgcn_aggregate(z(n, 9), graph, et, 3, comp=z(3, 2))
    with pytest.raises(ValueError, match="edge_type"):
        ops.rgcn_aggregate(z(n, 8), graph, et[:-1], 3, comp=z(3, 2))


# ---- the select form ---------------------------------------------------------------------------------------------------

def run_select(C, R, graph_name, aggr, dev):
    from rgb_experiment_amd import ops
    ei, n = H.graph_of(graph_name)
    graph = operator_graph(graph_name, dev)
    h, y0, cot = (t.float().to(dev) for t in H.select_case(C, R, graph_name))
    h, y0 = h.requires_grad_(True), y0.requires_grad_(True)
    et = device_types(graph_name, R, dev)
    ops.typed_view(graph, et, R).select                                   # the index sets, before the poison
    poison(dev, (n, C), (n * R, C))
    out = ops.rgcn_aggregate(h, graph, et, R, aggr=aggr, y0=y0)
    (out * cot).sum().backward()
    return out.detach(), [h.grad, y0.grad]


@pytest.mark.parametrize("C,R,graph,aggr", H.SELECT_CASES)
def test_select_forward_backward(dev, C, R, graph, aggr):
    out, grads = run_select(C, R, graph, aggr, dev)
    assert finite(out, *grads), "a row was left unwritten"
    want = H.select_reference(C, R, graph, aggr)
    assert close(out, want[0], FWD_TOL), "forward"
    for name, got, ref in zip(H.SELECT_NAMES[1:], grads, want[1]):
        assert got.shape == ref.shape and close(got, ref, GRAD_TOL), name
    if graph == "no_edges":
        assert torch.equal(out.cpu(), H.select_case(C, R, graph)[1].float()) and grads[0].abs().max().item() == 0.0
    again = run_select(C, R, graph, aggr, dev)
    assert torch.equal(out, again[0]) and all(torch.equal(a, b) for a, b in zip(grads, again[1]))


def test_select_index_sets(dev):
    """col' = col * R + type over the forward CSR; the relation-expanded transposed CSR has N * R rows and row j * R + r
    holds the out-edges of j with relation r."""
    from rgb_experiment_amd import ops
    for R in (1, 3):
        check_select_index_sets(R, dev)


def check_select_index_sets(R, dev):
    from rgb_experiment_amd import ops
    graph = operator_graph("powerlaw", dev)
    view = ops.typed_view(graph, device_types("powerlaw", R, dev), R)
    fwd, bwd, w_bwd = view.select
    E = graph.E
    assert torch.equal(fwd.col.long(), graph.fwd.col[:E].long() * R + view.etype_f.long()) and fwd.rowptr is graph.fwd.rowptr
    assert bwd.N == graph.N * R and bwd.nnz == E
    assert (bwd.split is not None) == (R == 1)          # one relation: the transposed CSR's own hub rows, and their plan
    ei = H.graph_of("powerlaw")[0]
    key = ei[0] * R + H.edge_type_of("powerlaw", R)
    assert torch.equal((bwd.rowptr[1:] - bwd.rowptr[:-1]).cpu().long(), torch.bincount(key, minlength=graph.N * R))
    order = torch.argsort(key, stable=True)
    assert torch.equal(bwd.col[:E].cpu().long(), ei[1][order])
    etype, cnt = H.slot_counts("powerlaw", R)
    inv = torch.empty_like(order)
    inv[H.slots_of("powerlaw")[3]] = torch.arange(E)
    assert torch.equal(w_bwd.cpu(), (1.0 / cnt.float())[inv[order]])


def test_select_form_refuses_an_index_range_beyond_int32(dev):
    """N * R >= 2^31: refused before any launch (the operand is a stride-0 view: no memory behind its 2^31 elements)."""
    from rgb_experiment_amd import ops
    N, R = 2 ** 28, 8
    h = torch.zeros(1, R, device=dev).expand(N, R)
    with pytest.raises(RuntimeError, match="beyond int32"):
        ops.rgcn_aggregate(h, H.HostGraph(N, 10), torch.zeros(10, dtype=torch.int64, device=dev), R)


# ---- layer ---------------------------------------------------------------------------------------------------------

def product_layer(name, ref, dev):
    C, kw = H.LAYER_CASES[name]
    conv = RGCNConv(H.LAYER_F, C, H.LAYER_R, **kw)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return conv.to(dev)


@pytest.mark.parametrize("name", sorted(H.LAYER_CASES))
def test_layer_forward_backward(dev, name):
    """Output, g_x and every parameter gradient against the restatement; width 67 is padded by the layer, 65 bases run
    the select form on composed weights."""
    x, ei, et, ref = H.layer_case(name)
    conv = product_layer(name, ref, dev)
    C, kw = H.LAYER_CASES[name]
    assert (conv.mix_channels() is None) == ("num_bases" not in kw or kw["num_bases"] > 64)
    assert (conv.mix_channels() not in (None, C)) == (C == H.PADDED_WIDTH)
    xd = x.float().to(dev).requires_grad_(True)
    out = conv(xd, ei.to(dev), et.to(dev))
    xr = x.clone().requires_grad_(True)
    want = ref(xr, ei, et)
    assert out.shape == want.shape and finite(out) and close(out, want, FWD_TOL), "forward"
    cot = T.f32_exact(want.shape, torch.Generator().manual_seed(17))
    (out * cot.float().to(dev)).sum().backward()
    (want * cot).sum().backward()
    assert close(xd.grad, xr.grad, GRAD_TOL), "g_x"
    refp, got = dict(ref.named_parameters()), dict(conv.named_parameters())
    assert sorted(got) == sorted(refp)
    for key, prm in got.items():
        assert prm.grad is not None and finite(prm.grad) and close(prm.grad, refp[key].grad, GRAD_TOL), key


def test_layer_follows_comp_and_edge_type_changed_in_place(dev):
    x, ei, et, ref = H.layer_case("bases")
    conv = product_layer("bases", ref, dev)
    xd, eid, etd = x.float().to(dev), ei.to(dev), et.to(dev)
    from rgb_experiment_amd.graph import LOOPS_KEEP, get_graph
    with torch.no_grad():
        a = conv(xd, eid, etd)
        conv.comp.mul_(-1.5)
        ref.comp.mul_(-1.5)
        b = conv(xd, eid, etd)
        assert not torch.equal(a, b) and close(b, ref(x, ei, et), FWD_TOL)
        views = get_graph(eid, xd.size(0), LOOPS_KEEP).__dict__["_typed_views"]
        assert len(views) == 1                                            # two forwards, one view
        etd.copy_((etd + 1) % H.LAYER_R)                                  # in place: the typed view is rebuilt
        c = conv(xd, eid, etd)
        assert len(views) == 2 and close(c, ref(x, ei, (et + 1) % H.LAYER_R), FWD_TOL)


# ---- model, experiment() ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_bases", [None, 3])
def test_model_against_restatement(dev, num_bases):
    """Logits, `emb` and every parameter gradient of one training step."""
    x, y, ei, et, model, ref = H.model_case(num_bases)
    model.to(dev).train()
    ref.train()
    res = model(x.float().to(dev), ei.to(dev), et.to(dev))
    want = ref(x, ei, et)
    assert {"out", "emb"} <= set(res.keys())
    assert close(res["emb"], want["emb"], FWD_TOL) and close(res["out"], want["out"], FWD_TOL)
    torch.nn.functional.nll_loss(res["out"], y.to(dev)).backward()
    torch.nn.functional.nll_loss(want["out"], y).backward()
    refp, got = dict(ref.named_parameters()), dict(model.named_parameters())
    assert sorted(got) == sorted(refp)
    for name, prm in got.items():
        assert prm.grad is not None and close(prm.grad, refp[name].grad, GRAD_TOL), name


@pytest.mark.parametrize("num_bases", [None, 2])
def test_experiment_trains_and_hip_graph_equals_eager(dev, num_bases):
    import rgb_experiment_amd as R
    n, f, c, rel, epochs = 300, 16, 4, 5, 5
    gen = torch.Generator().manual_seed(11)
    ei = rand_graph(n, 1800, 13, loops=4, dups=4)
    data = R.Data(x=torch.randn(n, f, generator=gen), y=torch.randint(0, c, (n,), generator=gen), edge_index=ei,
                  edge_type=torch.randint(0, rel, (ei.size(1),), generator=gen))
    params = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0, "num_relations": rel}
    if num_bases:
        params["num_bases"] = num_bases
    runs = []
    for graphed in (False, True, False):
        runs.append(R.experiment(params, specify_data=True, data=data, model_name="rgcn", learning_rate=0.01,
                                 epoch=epochs, need_to_reappear=True, print_print=False, return_model=True,
                                 use_hip_graph=graphed, implement_early_stopping=False, use_edge_type=True))
    a, b, a2 = runs
    assert isinstance(a["model"], RGCN)
    for key in ("ACC", "precision_score", "recall_score", "f1_macro", "f1_micro"):
        assert key in a and np.isfinite(float(a[key])), key
    assert b["used_hip_graph"] and not a["used_hip_graph"]
    assert len(a["history"]["train_loss"]) == epochs and len(b["history"]["train_loss"]) == epochs
    assert a["history"] == a2["history"]                                    # two seeded runs: bit-identical
    for key in ("train_loss", "val_loss", "test_loss"):                     # (the two loops divide the same sums on the
        assert np.allclose(a["history"][key], b["history"][key], rtol=0, atol=1e-6), key   # device and on the host)
    for key in ("train_acc", "val_acc", "test_acc"):
        assert a["history"][key] == b["history"][key], key
    sa, sb, sa2 = (r["model"].state_dict() for r in (a, b, a2))             # both loops train bit-identically
    assert sorted(sa) == sorted(sb) and all(torch.equal(sa[k], sb[k]) and torch.equal(sa[k], sa2[k]) for k in sa)
    assert a["history"]["train_loss"][-1] < a["history"]["train_loss"][0]
    if num_bases:                                                            # comp takes a gradient: it is trained
        for conv in a["model"].convs:
            assert conv.comp.grad is not None and conv.comp.grad.abs().max().item() > 0.0
    with pytest.raises(TypeError):                                           # flag off: the model's forward lacks its argument
        R.experiment(params, specify_data=True, data=data, model_name="rgcn", epoch=1, print_print=False,
                     use_hip_graph=False)
