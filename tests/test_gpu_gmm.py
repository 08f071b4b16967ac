"""GMMConv / MoNet on the MI355X: ops.gmm_aggregate (every vector width and group count of the lane layout, kernel counts
in one and in several head chunks, 1 to 8 pseudo-coordinates, hub rows in both CSRs, rows of exactly 0 / 1 / 64 / 65 / T /
T + 1 slots, a graph without edges, graphs of one to three nodes, the planted case, mean and sum, with and without y0) with
all five gradients, selective backward passes, strided and offset operands, bit-identical reruns, parameters moved in place,
ops.degree_pseudo, GMMConv, the MoNet model, experiment(model_name="monet") and a seeded differential fuzz, against the
float64 restatement of tests/test_gmm_host.py. The cases are that file's; it checks on the CPU that each is well-posed.

Tolerances are the project's: forward 1e-4 * max(1, |ref|max), gradients 2e-4 * max(1, |ref|max). Every element is
compared. Before every operator call the allocator's free blocks of the sizes the op allocates are filled with NaN
(`poison`), so a row or a slot that a kernel skipped shows as NaN instead of passing on stale zeros; `finite` is asserted
on top."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import test_gmm_host as H
import test_transformer_host as T
from test_gmm_host import GMMConv, MoNet
from test_gpu_ggnn import close, rand_graph
from test_gpu_transformer import device_graph, finite, poison

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


def workspace_floats(nnz, K, D):
    from rgb_experiment_amd import _lib
    n = ctypes.c_size_t(0)
    _lib.check(_lib.load().rgbx_gmm_bwd_edge_workspace_bytes(nnz, K, D, ctypes.byref(n)), "workspace")
    return max(n.value // 4, 1)


def run_gmm(tensors, ei, n, graph, aggr, with_y0, dev, needs=(True,) * 5, sink=None):
    """ops.gmm_aggregate: forward and the gradients asked for (`needs`: of h, e_slot, mu, sigma, y0). The attribute rows
    go in slot order; g_e comes back in slot order and is returned per INPUT edge, as the restatement has it."""
    from rgb_experiment_amd import ops
    h, e, mu, sigma, y0, cot = (t.float().to(dev) for t in tensors)
    K, D = mu.shape
    M = h.size(1) // K
    E = ei.size(1)
    order = graph.fwd.perm[:E].long() if E else torch.zeros(0, dtype=torch.int64, device=dev)
    e_slot = e[order].contiguous()
    h, e_slot, mu, sigma, y0 = (t.requires_grad_(need) for t, need in zip((h, e_slot, mu, sigma, y0), needs))
    graph.inv_deg, graph.w_mean_t, graph.t2f                              # built before the poison, as in a second step
    poison(dev, (n, M), (n, K * M), (max(E, 1), D), (K, D), (workspace_floats(E, K, D),))
    if sink is not None:
        ops.set_event_sink(sink)
    try:
        out = ops.gmm_aggregate(h, e_slot, mu, sigma, graph, aggr=aggr, y0=y0 if with_y0 else None)
        if any(needs[:4]) or (with_y0 and needs[4]):
            (out * cot).sum().backward()
    finally:
        ops.set_event_sink(None)
    g_e = None
    if e_slot.grad is not None:
        g_e = torch.empty_like(e_slot.grad)
        g_e[order] = e_slot.grad                                          # edge order[p] receives slot p's row
    return out.detach(), [h.grad, g_e, mu.grad, sigma.grad, y0.grad if with_y0 else None]


def run_case(K, M, D, graph_name, aggr, with_y0, dev, **kw):
    ei, n = H.graph_of(graph_name)
    return run_gmm(H.operator_case(K, M, D, graph_name), ei, n, operator_graph(graph_name, dev), aggr, with_y0, dev, **kw)


def compare(out, grads, want, cot):
    assert finite(out, *[g for g in grads if g is not None]), "a row or a slot was left unwritten"
    assert close(out, want[0], FWD_TOL), "forward"
    for name, got, ref in zip(H.NAMES[1:], grads, want[1]):
        if ref is None:
            assert got is None, name
            continue
        assert got is not None and got.shape == ref.shape, name
        assert ref.numel() == 0 or close(got, ref, GRAD_TOL), name
    if grads[4] is not None:
        assert torch.equal(grads[4].cpu(), cot.float())                   # g_y0 is the cotangent


@pytest.mark.parametrize("K,M,D,graph,aggr,with_y0", H.CASES)
def test_forward_backward(dev, K, M, D, graph, aggr, with_y0):
    from rgb_experiment_amd import ops
    assert ops.gmm_supported(K, M, D)
    out, grads = run_case(K, M, D, graph, aggr, with_y0, dev)
    case = H.operator_case(K, M, D, graph)
    compare(out, grads, H.reference(K, M, D, graph, aggr, with_y0), case[5])
    y0 = case[4].float() if with_y0 else torch.zeros_like(case[4]).float()
    if graph == "no_edges":
        assert torch.equal(out.cpu(), y0) and all(grads[i].abs().max().item() == 0.0 for i in (0, 2, 3))
        assert grads[1].shape == (0, D)
    if graph == "random":                 # rows without in-edges store y0; sources without out-edges get zeros
        assert torch.equal(out[:20].cpu(), y0[:20]) and grads[0][20:40].abs().max().item() == 0.0


def test_planted_case(dev):
    """The hand-derived numbers of tests/test_gmm_host.py: coefficients 1 and exp(-1/2), a duplicate, a self-loop, three
    targets without in-edges."""
    from rgb_experiment_amd import ops
    ei, n = H.graph_of("planted")
    graph = operator_graph("planted", dev)
    h, e, mu, sigma = (t.float().to(dev) for t in H.planted_case())
    e_slot = e[graph.fwd.perm[:ei.size(1)].long()].contiguous()
    for aggr in ("mean", "sum"):
        poison(dev, (n, 1))
        out = ops.gmm_aggregate(h, e_slot, mu, sigma, graph, aggr=aggr)
        want = torch.tensor(H.planted_expected(aggr), dtype=torch.float64)[:, None]
        assert finite(out) and close(out, want, FWD_TOL), aggr
        assert out[3:].abs().max().item() == 0.0 and out[0].item() == want[0].item()   # gauss = 1 exactly on mu_0


@pytest.mark.parametrize("graph", ["random", "powerlaw"])
def test_selective_passes(dev, graph):
    """Only h asks for a gradient: only the source pass is launched; e_slot, mu or sigma: only the edge pass; y0 alone:
    neither. What is computed has the bits of the full backward."""
    K, M, D = 8, 16, 2
    _, full = run_case(K, M, D, graph, "mean", True, dev)
    for needs, launched in (((True, False, False, False, False), ["gmm_fwd", "gmm_bwd_src"]),
                            ((False, True, False, False, False), ["gmm_fwd", "gmm_bwd_edge"]),
                            ((False, False, True, False, False), ["gmm_fwd", "gmm_bwd_edge"]),
                            ((False, False, False, True, False), ["gmm_fwd", "gmm_bwd_edge"]),
                            ((False, False, False, False, True), ["gmm_fwd"]),
                            ((False, False, False, False, False), ["gmm_fwd"]),
                            ((True,) * 5, ["gmm_fwd", "gmm_bwd_src", "gmm_bwd_edge"])):
        sink = []
        _, got = run_case(K, M, D, graph, "mean", True, dev, needs=needs, sink=sink)
        torch.cuda.synchronize()
        assert [str(kind) for kind, _, _ in sink if str(kind).startswith("gmm")] == launched
        for need, a, b in zip(needs, got, full):
            assert (a is None) == (not need) and (a is None or torch.equal(a, b))


def test_two_runs_are_bit_identical(dev):
    """No float atomics and fixed summation orders: forward and backward twice on the hub-row graph, same bits, the
    parameter gradients included."""
    for K, M, D in ((8, 16, 2), (2, 66, 3)):
        for aggr in ("mean", "sum"):
            (out_a, grads_a), (out_b, grads_b) = [run_case(K, M, D, "powerlaw", aggr, True, dev) for _ in range(2)]
            assert torch.equal(out_a, out_b) and all(torch.equal(a, b) for a, b in zip(grads_a, grads_b))
            assert grads_a[2].abs().max().item() > 0.0 and grads_a[3].abs().max().item() > 0.0


def test_strided_and_offset_operands(dev):
    """h, y0 and e_slot as column blocks of wider matrices and a column-major cotangent give the bits of contiguous
    operands; an h that starts off the 16-byte grid is read one float at a time (another order of the sums: the
    tolerances)."""
    from rgb_experiment_amd import ops
    K, M, D = 4, 64, 3
    graph = operator_graph("random", dev)
    ei, n = H.graph_of("random")
    h, e, mu, sigma, y0, cot = (t.float().to(dev) for t in H.operator_case(K, M, D, "random"))
    e = e[graph.fwd.perm[:ei.size(1)].long()].contiguous()
    F = K * M

    def run(hv, yv, ev, cotv, wide):
        hv, yv, ev = (t.detach().requires_grad_(True) for t in (hv, yv, ev))
        mv, sv = mu.detach().requires_grad_(True), sigma.detach().requires_grad_(True)
        hs, ys, es = (hv[:, 8:8 + F], yv[:, 4:4 + M], ev[:, 1:1 + D]) if wide else (hv, yv, ev)
        out = ops.gmm_aggregate(hs, es, mv, sv, graph, y0=ys)
        (out * cotv).sum().backward()
        grads = (hv.grad[:, 8:8 + F], yv.grad[:, 4:4 + M], ev.grad[:, 1:1 + D]) if wide else (hv.grad, yv.grad, ev.grad)
        return out.detach(), grads + (mv.grad, sv.grad)

    plain_out, plain_grads = run(h, y0, e, cot, False)
    pad = torch.nn.functional.pad
    wide_out, wide_grads = run(pad(h, (8, 8)), pad(y0, (4, 12)), pad(e, (1, 2)), cot.t().contiguous().t(), True)
    assert torch.equal(plain_out, wide_out)
    assert all(torch.equal(a, b) for a, b in zip(plain_grads, wide_grads))
    flat = torch.zeros(h.numel() + 1, device=dev)
    flat[1:] = h.reshape(-1)
    off_grid = flat[1:].view_as(h)
    assert off_grid.data_ptr() % 16 == 4
    off_out, off_grads = run(off_grid, y0, e, cot, False)
    assert close(off_out, plain_out.cpu().double(), FWD_TOL)
    assert all(close(a, b.cpu().double(), GRAD_TOL) for a, b in zip(off_grads, plain_grads))


def test_mu_and_sigma_are_read_on_the_device(dev):
    """mu changed in place between two forwards changes the output accordingly: nothing of it is cached on the host."""
    from rgb_experiment_amd import ops
    K, M, D = 3, 5, 2
    graph = operator_graph("random", dev)
    ei, n = H.graph_of("random")
    case = H.operator_case(K, M, D, "random")
    h, e, mu, sigma, y0, _ = (t.float().to(dev) for t in case)
    e_slot = e[graph.fwd.perm[:ei.size(1)].long()].contiguous()
    with torch.no_grad():
        a = ops.gmm_aggregate(h, e_slot, mu, sigma, graph, y0=y0)
        mu.add_(0.25)
        b = ops.gmm_aggregate(h, e_slot, mu, sigma, graph, y0=y0)
        sigma.mul_(-1.0)                                                   # only sigma^2 enters
        c = ops.gmm_aggregate(h, e_slot, mu, sigma, graph, y0=y0)
    assert not torch.equal(a, b) and torch.equal(b, c)
    moved = (case[0], case[1], case[2] + 0.25, case[3], case[4], case[5])
    assert close(b, H.run_formula(moved, "random", "mean")[0], FWD_TOL)


@pytest.mark.parametrize("name", H.graph_names + ("planted",))
def test_degree_pseudo(dev, name):
    """BIT FOR BIT against the host's 1.0 / sqrt((1 + indeg).float()): the kernel takes one correctly rounded float32
    square root and one correctly rounded float32 division of an exactly represented integer, as the host does. Cached."""
    from rgb_experiment_amd import ops
    ei, n = H.graph_of(name)
    graph = device_graph(ei.clone(), n, dev)                               # a graph of its own: nothing cached on it yet
    E = ei.size(1)
    poison(dev, (max(E, 1), 2))
    u = ops.degree_pseudo(graph)
    assert ops.degree_pseudo(graph) is u and u.shape == (E, 2) and u.dtype == torch.float32 and not u.requires_grad
    if E:
        assert finite(u)
        want = H.degree_pseudo(ei, n)[graph.fwd.perm[:E].cpu().long()]
        assert torch.equal(u.cpu(), want)


def test_operator_refusals(dev):
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_REMOVE_ADD, get_graph
    graph = operator_graph("random", dev)
    ei, n = H.graph_of("random")
    E = ei.size(1)
    z = lambda *s: torch.zeros(*s, device=dev)
    assert not ops.gmm_supported(2, 67, 2) and not ops.gmm_supported(65, 8, 2) and not ops.gmm_supported(2, 8, 9)
    with pytest.raises(RuntimeError, match="pad the width"):
        ops.gmm_aggregate(z(n, 2 * 67), z(E, 2), z(2, 2), z(2, 2), graph)
    with pytest.raises(RuntimeError, match="1 <= K <= 64"):
        ops.gmm_aggregate(z(n, 65 * 4), z(E, 2), z(65, 2), z(65, 2), graph)
    with pytest.raises(RuntimeError, match="1 <= D <= 8"):
        ops.gmm_aggregate(z(n, 8), z(E, 9), z(2, 9), z(2, 9), graph)
    with pytest.raises(RuntimeError, match="e_slot"):
        ops.gmm_aggregate(z(n, 8), z(E - 1, 2), z(2, 2), z(2, 2), graph)
    with pytest.raises(RuntimeError, match="LOOPS_KEEP"):
        ops.gmm_aggregate(z(n, 8), z(E, 2), z(2, 2), z(2, 2), get_graph(graph._keepalive, n, LOOPS_REMOVE_ADD))


# ---- layer ---------------------------------------------------------------------------------------------------------

def product_layer(name, ref, dev):
    M, D, K, kw = H.LAYER_CASES[name]
    conv = GMMConv(H.LAYER_F, M, D, K, **kw)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return conv.to(dev)


@pytest.mark.parametrize("name", sorted(H.LAYER_CASES))
def test_layer_forward_backward(dev, name):
    """Output, g_x, g_edge_attr and every parameter gradient against the restatement; width 67 is padded by the layer;
    root_weight and bias on and off; train and eval give the same bits (the layer draws nothing)."""
    x, ei, ea, ref = H.layer_case(name)
    conv = product_layer(name, ref, dev)
    M = H.LAYER_CASES[name][0]
    assert (conv.kernel_channels() != M) == (M == H.PADDED_WIDTH)
    xd = x.float().to(dev).requires_grad_(True)
    ead = ea.float().to(dev).requires_grad_(True)
    conv.train()
    out = conv(xd, ei.to(dev), ead)
    xr, ear = x.clone().requires_grad_(True), ea.clone().requires_grad_(True)
    want = ref(xr, ei, ear)
    assert out.shape == want.shape and finite(out) and close(out, want, FWD_TOL), "forward"
    cot = T.f32_exact(want.shape, torch.Generator().manual_seed(17))
    (out * cot.float().to(dev)).sum().backward()
    (want * cot).sum().backward()
    assert close(xd.grad, xr.grad, GRAD_TOL), "g_x"
    assert close(ead.grad, ear.grad, GRAD_TOL), "g_edge_attr"
    refp, got = dict(ref.named_parameters()), dict(conv.named_parameters())
    assert sorted(got) == sorted(refp)
    for key, prm in got.items():
        assert prm.grad is not None and finite(prm.grad) and close(prm.grad, refp[key].grad, GRAD_TOL), key
    conv.eval()
    with torch.no_grad():
        assert torch.equal(conv(xd, ei.to(dev), ead.detach()), out)


def test_layer_follows_parameters_and_attributes_changed_in_place(dev):
    x, ei, ea, ref = H.layer_case("plain")
    conv = product_layer("plain", ref, dev)
    xd, eid, ead = x.float().to(dev), ei.to(dev), ea.float().to(dev)
    from rgb_experiment_amd.graph import LOOPS_KEEP, get_graph
    with torch.no_grad():
        a = conv(xd, eid, ead)
        conv.mu.add_(0.5)
        ref.mu.add_(0.5)
        b = conv(xd, eid, ead)
        assert not torch.equal(a, b) and close(b, ref(x, ei, ea), FWD_TOL)
        slots = get_graph(eid, xd.size(0), LOOPS_KEEP).__dict__["_edge_slots"]
        assert len(slots) == 1                                            # two forwards, one permuted copy
        ead.mul_(0.5)                                                     # in place: the copy is rebuilt
        c = conv(xd, eid, ead)
        assert len(slots) == 2 and close(c, ref(x, ei, ea * 0.5), FWD_TOL)


# ---- model, experiment() ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_attr", [True, False])
def test_model_against_restatement(dev, with_attr):
    """Logits, `emb` and every parameter gradient of one training step, with edge attributes and with the degree
    pseudo-coordinates."""
    x, y, ei, ea, model, ref = H.model_case()
    model.to(dev).train()
    ref.train()
    res = model(x.float().to(dev), ei.to(dev), ea.float().to(dev) if with_attr else None)
    want = ref(x, ei, ea if with_attr else None)
    assert {"out", "emb"} <= set(res.keys())
    assert close(res["emb"], want["emb"], FWD_TOL) and close(res["out"], want["out"], FWD_TOL)
    torch.nn.functional.nll_loss(res["out"], y.to(dev)).backward()
    torch.nn.functional.nll_loss(want["out"], y).backward()
    refp, got = dict(ref.named_parameters()), dict(model.named_parameters())
    assert sorted(got) == sorted(refp)
    for name, prm in got.items():
        assert prm.grad is not None and close(prm.grad, refp[name].grad, GRAD_TOL), name


@pytest.mark.parametrize("use_edge_attr", [False, True])
def test_experiment_trains_and_hip_graph_equals_eager(dev, use_edge_attr):
    import rgb_experiment_amd as R
    n, f, c, epochs = 300, 16, 4, 5
    gen = torch.Generator().manual_seed(11)
    ei = rand_graph(n, 1800, 13, loops=4, dups=4)
    data = R.Data(x=torch.randn(n, f, generator=gen), y=torch.randint(0, c, (n,), generator=gen), edge_index=ei,
                  edge_attr=torch.rand(ei.size(1), 3, generator=gen))
    params = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0, "kernel_size": 3, "dim": 3 if use_edge_attr else 2}
    runs = []
    for graphed in (False, True, False):
        runs.append(R.experiment(params, specify_data=True, data=data, model_name="monet", learning_rate=0.01,
                                 epoch=epochs, need_to_reappear=True, print_print=False, return_model=True,
                                 use_hip_graph=graphed, implement_early_stopping=False, use_edge_attr=use_edge_attr))
    a, b, a2 = runs
    assert isinstance(a["model"], MoNet)
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
    for conv in a["model"].convs:                                            # mu and sigma take a gradient: they are trained
        assert conv.mu.grad is not None and conv.mu.grad.abs().max().item() > 0.0
        assert conv.sigma.grad is not None and conv.sigma.grad.abs().max().item() > 0.0


# ---- the seeded differential fuzz ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", H.FUZZ_SEEDS)
def test_fuzz_against_the_restatement(dev, seed):
    """K, M, n and the degrees drawn from the lists of tests/test_gpu_fuzz_families.py, D from 1 .. 8; the host file checks
    that every seed is supported and well-posed."""
    K, M, D, aggr, with_y0, ei, n, case = H.fuzz_case(seed)
    graph = device_graph(ei, n, dev)
    assert graph.fwd.nnz == ei.size(1)
    out, grads = run_gmm(case, ei, n, graph, aggr, with_y0, dev)
    compare(out, grads, H.run_fuzz(seed), case[5])
