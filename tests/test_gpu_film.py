"""FiLMConv on the MI355X: ops.film_aggregate (every vector width of the lane layout, one / three / seven relations, mean
and add, relu and identity, hub rows in the plain and in both relation-expanded CSRs, rows of exactly 0 / 1 / 64 / 65 / T /
T + 1 slots, a graph without edges, graphs of one to three nodes, the planted graph with its exact-zero gradient
entries, a width above 256 through the column cut), the relation-expanded index sets of the typed view, selective
backward passes, strided and offset operands, bit-identical reruns, FiLMConv, the FiLM model and
experiment(model_name="film"), against the float64 restatement of tests/test_film_host.py. The cases are that file's; it
checks on the CPU that each is well-posed.

Tolerances are the project's: forward 1e-4 * max(1, |ref|max), gradients 2e-4 * max(1, |ref|max). Every element is
compared. Before every operator call the allocator's free blocks of the sizes the op allocates are filled with NaN
(`poison`), so a row that a kernel skipped shows as NaN instead of passing on stale zeros; `finite` is asserted on top."""
import functools

import numpy as np
import pytest
import torch

import test_film_host as H
import test_transformer_host as T
from test_film_host import FiLM, FiLMConv
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


@functools.lru_cache(maxsize=None)
def device_types(name, R, dev):
    """The host file's edge types on the device: ONE tensor per (graph, R), so the typed view is built once."""
    return H.edge_type_of(name, R).to(dev)


# ---- the relation-expanded index sets -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["degrees", "powerlaw", "random", "no_edges", "planted"])
def test_expanded_index_sets(dev, name):
    """expand_fwd: N * R rows, row i * R + r holds the sources of the in-edges of i with relation r in edge order; the
    source pass shares select's expanded transposed CSR. Row lengths are the counts behind the mean weights. On `degrees`
    each of the two has exactly one hub row under every R, with a plan of its own."""
    from rgb_experiment_amd import ops
    graph = operator_graph(name, dev)
    ei, n = H.graph_of(name)
    for R in ((H.PLANTED_R,) if name == "planted" else H.RELATIONS):
        et = device_types(name, R, dev)
        view = ops.typed_view(graph, et, R)
        exp = view.expand_fwd
        assert view.expand_fwd is exp                                      # built once per view
        if R == 1:
            assert exp is graph.fwd                                        # one relation: the plain forward CSR
            continue
        bwd = view.select[1]
        assert exp.N == n * R and exp.nnz == ei.size(1) and bwd.N == n * R
        fin, fout = H.expanded_lengths(name, R)
        assert torch.equal((exp.rowptr[1:] - exp.rowptr[:-1]).cpu().long(), fin)
        assert torch.equal((bwd.rowptr[1:] - bwd.rowptr[:-1]).cpu().long(), fout)
        if ei.size(1):
            key = ei[1] * R + H.edge_type_of(name, R)
            assert torch.equal(exp.col[:exp.nnz].cpu().long(), ei[0][torch.argsort(key, stable=True)])
        if name == "degrees":
            assert exp.split is not None and exp.split["n_long"] == 1 and exp.split["n_chunks"] == 2
            assert bwd.split is not None and bwd.split["n_long"] == 1
            lens = set(fin.tolist())
            assert set(H.G.DEGREES) <= lens and set(H.G.DEGREES) <= set(fout.tolist())
        if name == "random":
            assert exp.split is None


def test_expanded_set_is_rebuilt_when_edge_type_changes_in_place(dev):
    from rgb_experiment_amd import ops
    graph = operator_graph("random", dev)
    ei, n = H.graph_of("random")
    et = H.edge_type_of("random", 3).to(dev)                              # a tensor of its own: it is edited below
    a = ops.typed_view(graph, et, 3)
    ea = a.expand_fwd
    assert ops.typed_view(graph, et, 3).expand_fwd is ea                  # cached with the view
    et.copy_((et + 1) % 3)                                                # in place: the version moves, the view is rebuilt
    b = ops.typed_view(graph, et, 3)
    assert b is not a and b.expand_fwd is not ea
    key = ei[1] * 3 + (H.edge_type_of("random", 3) + 1) % 3
    assert torch.equal((b.expand_fwd.rowptr[1:] - b.expand_fwd.rowptr[:-1]).cpu().long(), torch.bincount(key, minlength=3 * n))


def test_the_operand_range_beyond_int32_is_refused(dev):
    """N * R >= 2^31: refused before any launch (the operands are stride-0 views: no memory behind their elements)."""
    from rgb_experiment_amd import ops
    N, R = 2 ** 28, 8
    h = torch.zeros(1, R, device=dev).expand(N, R)
    fb = torch.zeros(1, 2 * R, device=dev).expand(N, 2 * R)
    with pytest.raises(RuntimeError, match="beyond int32"):
        ops.film_aggregate(h, fb, H.HostGraph(N, 10), torch.zeros(10, dtype=torch.int64, device=dev), R)


# ---- the operator ------------------------------------------------------------------------------------------------------

def run_op(C, R, graph_name, aggr, act, dev, needs=(True, True, True), sink=None, typed=True):
    """ops.film_aggregate: forward and the gradients asked for (`needs`: of h, fb, y0). `typed=False` (R = 1 only): the
    call without edge types, which needs no typed view."""
    from rgb_experiment_amd import ops
    ei, n = H.graph_of(graph_name)
    graph = operator_graph(graph_name, dev)
    h, fb, y0, cot = (t.float().to(dev) for t in H.operator_case(C, R, graph_name)[:4])
    h, fb, y0 = (t.requires_grad_(need) for t, need in zip((h, fb, y0), needs))
    et = device_types(graph_name, R, dev) if typed else None
    if typed:   # the index sets are built before the poison, as in a second step
        view = ops.typed_view(graph, et, R)
        view.select, view.expand_fwd
    graph.bwd
    Cb = min(C, 256)
    poison(dev, (n, Cb), (n * R, Cb), (n * R, 2 * Cb), (n, C), (n * R, C), (n * R, 2 * C))
    if sink is not None:
        ops.set_event_sink(sink)
    try:
        out = ops.film_aggregate(h, fb, graph, et, R, aggr=aggr, act=act, y0=y0)
        if any(needs):
            (out * cot).sum().backward()
    finally:
        ops.set_event_sink(None)
    return out.detach(), [h.grad, fb.grad, y0.grad]


def check_op(C, R, graph_name, aggr, act, dev, typed=True):
    out, grads = run_op(C, R, graph_name, aggr, act, dev, typed=typed)
    assert finite(out, *grads), "a row was left unwritten"
    want = H.reference(C, R, graph_name, aggr, act)
    assert close(out, want[0], FWD_TOL), "forward"
    for name, got, ref in zip(H.NAMES[1:], grads, want[1]):
        assert got.shape == ref.shape and close(got, ref, GRAD_TOL), name
    case = H.operator_case(C, R, graph_name)
    y0, n = case[2].float(), H.graph_of(graph_name)[1]
    assert torch.equal(grads[2].cpu(), case[3].float())                   # g_y0 is the cotangent
    if graph_name == "no_edges":   # out == y0 bit for bit, and nothing flows to h or fb
        assert torch.equal(out.cpu(), y0) and grads[0].abs().max().item() == 0.0 and grads[1].abs().max().item() == 0.0
    if graph_name == "random":     # rows without in-edges store y0; sources without out-edges get zeros
        assert torch.equal(out[:20].cpu(), y0[:20]) and grads[0].view(n, R, C)[20:40].abs().max().item() == 0.0
        assert grads[1].view(n, R, 2 * C)[:20].abs().max().item() == 0.0
    if R > 1 and graph_name != "planted":   # the relation without an edge
        assert grads[0].view(n, R, C)[:, R - 1].abs().max().item() == 0.0
        assert grads[1].view(n, R, 2 * C)[:, R - 1].abs().max().item() == 0.0
    if graph_name == "planted":
        assert torch.equal(out[4:].cpu(), y0[4:])                         # no in-edge: out == y0
        if act == "relu":          # the tie z == 0 and the z < 0: exact zeros, relu'(0) = 0
            gh, gfb = grads[0].view(6, H.PLANTED_R, C), grads[1].view(6, H.PLANTED_R, 2 * C)
            assert gh[0, 0].abs().max().item() == 0.0 and gfb[1, 0].abs().max().item() == 0.0
            assert gfb[1, 2].abs().max().item() == 0.0 and gfb[:, 3].abs().max().item() == 0.0
    if act == "relu" and case[4].numel():   # every planted tie contributes an exact zero: masked sums stay finite
        assert int(case[4].sum()) > 0
    return out, grads


@pytest.mark.parametrize("C,R,graph,aggr,act", H.CASES)
def test_forward_backward(dev, C, R, graph, aggr, act):
    from rgb_experiment_amd import ops
    assert ops.film_supported(min(C, 256))
    check_op(C, R, graph, aggr, act, dev)
    if R == 1:   # the single-relation call: no edge types, no typed view, weights from the row lengths
        check_op(C, R, graph, aggr, act, dev, typed=False)


def test_cases_cover_the_layout():
    vec = lambda C: 4 if C % 4 == 0 else (2 if C % 2 == 0 else 1)
    for graph in ("degrees", "powerlaw"):
        assert {vec(C) for C, _, g, _, _ in H.CASES if g == graph} == {1, 2, 4}
        assert {R for _, R, g, _, _ in H.CASES if g == graph} == set(H.RELATIONS)
    assert {(C, R) for C, R, g, _, _ in H.CASES if g == "degrees"} >= {(C, R) for C in H.WIDTHS for R in H.RELATIONS}


def test_sum_is_add_and_identity_is_none(dev):
    a = run_op(7, 3, "random", "add", "identity", dev)
    b = run_op(7, 3, "random", "sum", None, dev)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def test_without_y0_empty_rows_store_zeros(dev):
    from rgb_experiment_amd import ops
    graph = operator_graph("random", dev)
    h, fb, y0 = (t.float().to(dev) for t in H.operator_case(7, 3, "random")[:3])
    et = device_types("random", 3, dev)
    _, n = H.graph_of("random")
    poison(dev, (n, 7))
    with torch.no_grad():
        bare = ops.film_aggregate(h, fb, graph, et, 3)
        full = ops.film_aggregate(h, fb, graph, et, 3, y0=y0)
    assert finite(bare) and bare[:20].abs().max().item() == 0.0
    assert close(full - bare, y0.cpu().double(), FWD_TOL)


@pytest.mark.parametrize("graph,R", [("random", 3), ("powerlaw", 1), ("degrees", 7)])
def test_selective_passes(dev, graph, R):
    """Only h asks for a gradient: only the source pass is launched; only fb: only the film pass; y0 alone or nothing:
    neither. What is computed has the bits of the full backward."""
    C = 16
    _, full = run_op(C, R, graph, "mean", "relu", dev)
    for needs, launched in (((True, False, False), ["film_fwd", "film_bwd_src"]),
                            ((False, True, False), ["film_fwd", "film_bwd_film"]),
                            ((False, False, True), ["film_fwd"]),
                            ((False, False, False), ["film_fwd"]),
                            ((True, True, True), ["film_fwd", "film_bwd_src", "film_bwd_film"])):
        sink = []
        _, got = run_op(C, R, graph, "mean", "relu", dev, needs=needs, sink=sink)
        torch.cuda.synchronize()
        assert [str(kind) for kind, _, _ in sink if str(kind).startswith("film")] == launched
        for need, a, b in zip(needs, got, full):
            assert (a is None) == (not need) and (a is None or torch.equal(a, b))


def test_a_width_above_256_runs_as_column_blocks(dev):
    """300 channels: blocks of 256 and 44, each its own launches; the result is that of the blocks run one by one."""
    from rgb_experiment_amd import ops
    sink = []
    out, grads = run_op(H.BLOCKED_WIDTH, 3, "random", "mean", "relu", dev, sink=sink)
    torch.cuda.synchronize()
    kinds = [str(kind) for kind, _, _ in sink if str(kind).startswith("film")]
    assert sorted(kinds) == sorted(2 * ["film_fwd", "film_bwd_src", "film_bwd_film"])
    graph, et = operator_graph("random", dev), device_types("random", 3, dev)
    n, C, R = graph.N, H.BLOCKED_WIDTH, 3
    h, fb, y0 = (t.float().to(dev) for t in H.operator_case(C, R, "random")[:3])
    hv, fv = h.view(n, R, C), fb.view(n, R, 2 * C)
    with torch.no_grad():
        for a, b in ((0, 256), (256, 300)):
            blk = ops.film_aggregate(hv[:, :, a:b].reshape(n, -1),
                                     torch.cat([fv[:, :, a:b], fv[:, :, C + a:C + b]], dim=2).reshape(n, -1), graph, et, R,
                                     y0=y0[:, a:b].contiguous())
            assert torch.equal(blk, out[:, a:b])
    with pytest.raises(RuntimeError, match="pad the width"):
        ops.film_aggregate(torch.zeros(n, 67, device=dev), torch.zeros(n, 134, device=dev), graph)
    with pytest.raises(RuntimeError, match="pad the width"):
        ops.film_aggregate(torch.zeros(n, 323, device=dev), torch.zeros(n, 646, device=dev), graph)   # 256 and 67


def test_two_runs_are_bit_identical(dev):
    """No float atomics and fixed summation orders: all three kernels twice on the hub-row graphs, same bits."""
    for C, R, graph, typed in ((64, 1, "powerlaw", True), (64, 1, "powerlaw", False), (66, 7, "powerlaw", True),
                               (16, 3, "degrees", True)):
        (out_a, grads_a), (out_b, grads_b) = [run_op(C, R, graph, "mean", "relu", dev, typed=typed) for _ in range(2)]
        assert torch.equal(out_a, out_b) and all(torch.equal(a, b) for a, b in zip(grads_a, grads_b))


def test_strided_and_offset_operands(dev):
    """One relation: h, fb and y0 as column blocks of wider matrices and a column-major cotangent are taken as they are
    and give the bits of contiguous operands; so do the copies several relations need. An h that starts off the 16-byte
    grid is read one float at a time (another order of the sums: the tolerances)."""
    from rgb_experiment_amd import ops
    pad = torch.nn.functional.pad
    for R, typed in ((1, False), (1, True), (3, True)):
        C = 64
        graph = operator_graph("random", dev)
        et = device_types("random", R, dev) if typed else None
        h, fb, y0, cot = (t.float().to(dev) for t in H.operator_case(C, R, "random")[:4])

        def run(hv, fv, yv, cotv, wide):
            hv, fv, yv = (t.detach().requires_grad_(True) for t in (hv, fv, yv))
            hs, fs, ys = (hv[:, 8:8 + R * C], fv[:, 4:4 + 2 * R * C], yv[:, 4:4 + C]) if wide else (hv, fv, yv)
            out = ops.film_aggregate(hs, fs, graph, et, R, y0=ys)
            (out * cotv).sum().backward()
            grads = (hv.grad[:, 8:8 + R * C], fv.grad[:, 4:4 + 2 * R * C], yv.grad[:, 4:4 + C]) if wide else \
                (hv.grad, fv.grad, yv.grad)
            return out.detach(), grads

        plain_out, plain_grads = run(h, fb, y0, cot, False)
        wide_out, wide_grads = run(pad(h, (8, 8)), pad(fb, (4, 12)), pad(y0, (4, 12)), cot.t().contiguous().t(), True)
        assert torch.equal(plain_out, wide_out)
        assert all(torch.equal(a, b) for a, b in zip(plain_grads, wide_grads))
        flat = torch.zeros(h.numel() + 1, device=dev)
        flat[1:] = h.reshape(-1)
        off_grid = flat[1:].view_as(h)
        assert off_grid.data_ptr() % 16 == 4
        off_out, off_grads = run(off_grid, fb, y0, cot, False)
        assert close(off_out, plain_out.cpu().double(), FWD_TOL)
        assert all(close(a, b.cpu().double(), GRAD_TOL) for a, b in zip(off_grads, plain_grads))


def test_raw_wrappers(dev):
    """film_fwd_raw / film_bwd_raw on the [N * R, .] views give the bits of the autograd node; a beta-to-gamma view of a
    wider fb (gamma offset = the full width) is read in place and its gradient keeps the columns between at zero."""
    from rgb_experiment_amd import ops
    C, R = 16, 3
    graph, et = operator_graph("random", dev), device_types("random", R, dev)
    n = graph.N
    out, grads = run_op(C, R, "random", "mean", "relu", dev)
    h, fb, y0, cot = (t.float().to(dev) for t in H.operator_case(C, R, "random")[:4])
    view = ops.typed_view(graph, et, R)
    hv, fv = h.view(n * R, C), fb.view(n * R, 2 * C)
    poison(dev, (n, C), (n * R, C), (n * R, 2 * C))
    raw = ops.film_fwd_raw(hv, fv, C, graph, view, 1, 1, y0)
    g_h, g_fb = ops.film_bwd_raw(hv, fv, C, cot, graph, view, 1, 1)
    assert torch.equal(raw, out) and torch.equal(g_h.view(n, R * C), grads[0]) and torch.equal(g_fb.view(n, -1), grads[1])
    only_h = ops.film_bwd_raw(hv, fv, C, cot, graph, view, 1, 1, want_fb=False)
    assert only_h[1] is None and torch.equal(only_h[0], g_h)
    # channels 4 .. 11 as a block: h's columns, and fb from beta's column 4 to gamma's column 12, gamma offset C
    # (an 8-wide block sits on other lanes than 8 of 16 columns: compared with the same block as matrices of its own)
    a, b = 4, 12
    hc, fc = hv[:, a:b].contiguous(), torch.cat([fv[:, a:b], fv[:, C + a:C + b]], dim=1)
    yc, cc = y0[:, a:b].contiguous(), cot[:, a:b].contiguous()
    own_out = ops.film_fwd_raw(hc, fc, b - a, graph, view, 1, 1, yc)
    own_h, own_f = ops.film_bwd_raw(hc, fc, b - a, cc, graph, view, 1, 1)
    assert close(own_out, out[:, a:b].cpu().double(), FWD_TOL)
    poison(dev, (n, b - a), (n * R, b - a), (n * R, C + b - a))
    blk_out = ops.film_fwd_raw(hv[:, a:b], fv[:, a:C + b], C, graph, view, 1, 1, y0[:, a:b])
    assert torch.equal(blk_out, own_out)
    bh, bf = ops.film_bwd_raw(hv[:, a:b], fv[:, a:C + b], C, cc, graph, view, 1, 1)
    assert torch.equal(bh, own_h) and bf.shape == (n * R, C + b - a)
    assert torch.equal(bf[:, :b - a], own_f[:, :b - a]) and torch.equal(bf[:, C:], own_f[:, b - a:])
    assert bf[:, b - a:C].abs().max().item() == 0.0


# ---- layer ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(H.LAYER_CASES))
def test_layer_forward_backward(dev, name):
    """Output, g_x and every parameter gradient against the restatement; width 67 is padded by the layer; a custom `nn`
    computes the film rows."""
    x, ei, et, ref = H.layer_case(name)
    conv = H.product_layer(name, ref).to(dev)
    C = H.LAYER_CASES[name][0]
    assert (conv.kernel_channels() != C) == (C == H.PADDED_WIDTH)
    xd = x.float().to(dev).requires_grad_(True)
    out = conv(xd, ei.to(dev), None if et is None else et.to(dev))
    xr = x.clone().requires_grad_(True)
    want = ref(xr, ei, et)
    assert out.shape == want.shape and finite(out) and close(out, want, FWD_TOL), "forward"
    empty = (torch.bincount(ei[1], minlength=H.LAYER_N) == 0).nonzero(as_tuple=True)[0]
    fs = ref.film_skip(x)
    skip = H.activation(fs[:, C:] * ref.lin_skip(x) + fs[:, :C], ref.act).detach()
    assert empty.numel() > 0 and close(out[empty.to(dev)], skip[empty], FWD_TOL)   # no in-edge: the skip term alone
    cot = T.f32_exact(want.shape, torch.Generator().manual_seed(17))
    (out * cot.float().to(dev)).sum().backward()
    (want * cot).sum().backward()
    assert close(xd.grad, xr.grad, GRAD_TOL), "g_x"
    refp, got = dict(ref.named_parameters()), dict(conv.named_parameters())
    assert sorted(got) == sorted(refp)
    for key, prm in got.items():
        assert prm.grad is not None and finite(prm.grad) and close(prm.grad, refp[key].grad, GRAD_TOL), key


def test_layer_with_one_relation_ignores_edge_type_and_follows_edits(dev):
    from rgb_experiment_amd.graph import LOOPS_KEEP, get_graph
    x, ei, et, ref = H.layer_case("one_relation")
    conv = H.product_layer("one_relation", ref).to(dev)
    xd, eid = x.float().to(dev), ei.to(dev)
    with torch.no_grad():
        a = conv(xd, eid)
        b = conv(xd, eid, torch.full((ei.size(1),), 5, dtype=torch.int64, device=dev))   # one relation: not even read
        assert torch.equal(a, b) and "_typed_views" not in get_graph(eid, xd.size(0), LOOPS_KEEP).__dict__
    x3, ei3, et3, ref3 = H.layer_case("typed")
    conv3 = H.product_layer("typed", ref3).to(dev)
    etd = et3.to(dev)
    with torch.no_grad():
        conv3(x3.float().to(dev), ei3.to(dev), etd)
        etd.copy_((etd + 1) % H.LAYER_R)                                  # in place: the typed view is rebuilt
        c = conv3(x3.float().to(dev), ei3.to(dev), etd)
        assert close(c, ref3(x3, ei3, (et3 + 1) % H.LAYER_R), FWD_TOL)


# ---- model, experiment() ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", H.MODEL_RELATIONS)
def test_model_against_restatement(dev, R):
    """Logits, `emb` and every parameter gradient of one training step."""
    x, y, ei, et, model, ref = H.model_case(R)
    model.to(dev).train()
    ref.train()
    args = (ei.to(dev),) if et is None else (ei.to(dev), et.to(dev))
    res = model(x.float().to(dev), *args)
    want = ref(x, ei, et)
    assert {"out", "emb"} <= set(res.keys())
    assert close(res["emb"], want["emb"], FWD_TOL) and close(res["out"], want["out"], FWD_TOL)
    torch.nn.functional.nll_loss(res["out"], y.to(dev)).backward()
    torch.nn.functional.nll_loss(want["out"], y).backward()
    refp, got = dict(ref.named_parameters()), dict(model.named_parameters())
    assert sorted(got) == sorted(refp)
    for name, prm in got.items():
        assert prm.grad is not None and close(prm.grad, refp[name].grad, GRAD_TOL), name


@pytest.mark.parametrize("typed", [False, True])
def test_experiment_trains_and_hip_graph_equals_eager(dev, typed):
    import rgb_experiment_amd as R
    n, f, c, rel, epochs = 300, 16, 4, 5, 5
    gen = torch.Generator().manual_seed(11)
    ei = rand_graph(n, 1800, 13, loops=4, dups=4)
    data = R.Data(x=torch.randn(n, f, generator=gen), y=torch.randint(0, c, (n,), generator=gen), edge_index=ei,
                  edge_type=torch.randint(0, rel, (ei.size(1),), generator=gen))
    params = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0}
    if typed:
        params["num_relations"] = rel
    runs = []
    for graphed in (False, True, False):
        runs.append(R.experiment(params, specify_data=True, data=data, model_name="film", learning_rate=0.01,
                                 epoch=epochs, need_to_reappear=True, print_print=False, return_model=True,
                                 use_hip_graph=graphed, implement_early_stopping=False, use_edge_type=typed))
    a, b, a2 = runs
    assert isinstance(a["model"], FiLM) and all(conv.num_relations == (rel if typed else 1) for conv in a["model"].convs)
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
    for conv in a["model"].convs:                                            # the film rows take a gradient: they train
        assert conv.films[0].weight.grad is not None and conv.films[0].weight.grad.abs().max().item() > 0.0
    if typed:
        with pytest.raises(ValueError, match="edge_type"):                   # flag off: the layers miss their argument
            R.experiment(params, specify_data=True, data=data, model_name="film", epoch=1, print_print=False,
                         use_hip_graph=False)
