"""max / min / sum neighbourhood aggregation on the host: the `aggr` keyword of SAGEConv / MySAGEConv / GraphSAGE /
GraphSAGE2 and experiment(), every refusal, the C ABI's argument checks (before any launch), and the float64
restatement that tests/test_gpu_extremum.py measures the kernels against — pinned here to torch.scatter_reduce. No GPU
needed.

The restatement (first_extremal_slot / ref_extremum) works on a CSR given as rowptr / col: per (row, channel) the FIRST
slot that holds the row's extremum, the forward as the gather x[col[arg], c] (0 where a row has no slot), gradients from
torch autograd through that gather. On the GPU the CSR is the device's own, copied to the host; here it is built by a
stable sort of the edge list by target, which is what the device build does (include/rgbx_hip.h, rgbx_csr_build)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AGGRS = ("mean", "max", "min", "add", "sum")
NEW_ENTRIES = ("rgbx_spmm_csr_extremum_supported", "rgbx_spmm_csr_extremum_f32", "rgbx_extremum_bwd_f32")


# ---- the float64 restatement -------------------------------------------------------------------------------------------

def first_extremal_slot(rowptr, col, x, mode):
    """int64 [n, d]: per (row, channel) the lowest slot p of the row with x[col[p], c] equal to the row's extremum; -1 for
    rows without slots. Plain comparisons on the values as given (no arithmetic, so nothing is rounded)."""
    n, d = rowptr.numel() - 1, x.size(1)
    arg = torch.full((n, d), -1, dtype=torch.int64)
    ptr = rowptr.tolist()
    with torch.no_grad():
        for i in range(n):
            s, e = ptr[i], ptr[i + 1]
            if e == s:
                continue
            seg = x[col[s:e].long()]  # [deg, d]
            best = seg.max(0).values if mode == "max" else seg.min(0).values
            slots = torch.arange(s, e)[:, None].expand(-1, d)
            arg[i] = torch.where(seg == best[None, :], slots, torch.full_like(slots, e)).min(0).values
    return arg


def ref_extremum(rowptr, col, x, mode):
    """(out [n, d], arg): out[i, c] = x[col[arg[i, c]], c], 0 where arg = -1; differentiable in x through the gather."""
    arg = first_extremal_slot(rowptr, col, x.detach(), mode)
    if not col.numel():  # a graph without edges: every row is empty
        return x.new_zeros(arg.shape), arg
    src = col.long()[arg.clamp(min=0)]  # [n, d] source node per (row, channel)
    out = torch.gather(x, 0, src) if x.size(0) else x.new_zeros(arg.shape)
    return torch.where(arg >= 0, out, torch.zeros_like(out)), arg


def ref_sum(rowptr, col, x):
    n = rowptr.numel() - 1
    row = torch.repeat_interleave(torch.arange(n), (rowptr[1:] - rowptr[:-1]).long())
    return torch.zeros((n, x.size(1)), dtype=x.dtype).index_add(0, row, x[col.long()])


def ref_aggregate(rowptr, col, x, aggr):
    if aggr in ("max", "min"):
        return ref_extremum(rowptr, col, x, aggr)[0]
    out = ref_sum(rowptr, col, x)
    if aggr == "mean":
        out = out / (rowptr[1:] - rowptr[:-1]).clamp(min=1).to(x.dtype)[:, None]
    return out


def host_csr(edge_index, n, loops="keep"):
    """(rowptr, col) of the target-grouped CSR of `edge_index`, slots in edge order within a row (stable sort).
    loops='remove_add': self-loops dropped, one per node appended (nodes ascending) — rgbx_csr_build's rewrite."""
    src, dst = edge_index[0], edge_index[1]
    if loops == "remove_add":
        keep = src != dst
        every = torch.arange(n)
        src, dst = torch.cat([src[keep], every]), torch.cat([dst[keep], every])
    order = torch.argsort(dst, stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
    return rowptr, src[order]


class RefSAGEConv(torch.nn.Module):
    """float64 twin of nn.SAGEConv (my=False: PyG's order — aggregate x, lin_l(agg) + lin_r(x)) and nn.MySAGEConv
    (my=True: the reference's order — lin_l, lin_r, aggregate x_l, += x_r; models/graphsage.py:49-60) over a CSR given
    to forward as (rowptr, col): same parameter names as the layers."""

    def __init__(self, cin, cout, aggr, my):
        super().__init__()
        self.aggr, self.my = ("add" if aggr == "sum" else aggr), my
        self.lin_l = torch.nn.Linear(cin, cout, bias=True).double()
        self.lin_r = torch.nn.Linear(cin, cout, bias=my).double()

    def forward(self, x, csr):
        if self.my:
            return ref_aggregate(csr[0], csr[1], self.lin_l(x), self.aggr) + self.lin_r(x)
        return self.lin_l(ref_aggregate(csr[0], csr[1], x, self.aggr)) + self.lin_r(x)


class RefSAGEStack(torch.nn.Module):
    """(conv -> BatchNorm1d) x (L-1), conv: the ConvStack skeleton in float64 with the state_dict keys of GraphSAGE /
    GraphSAGE2. Returns the logits."""

    def __init__(self, num_layers, hidden, cin, cout, aggr, my):
        super().__init__()
        widths = [cin] + [hidden] * (num_layers - 1) + [cout]
        self.convs = torch.nn.ModuleList(RefSAGEConv(widths[i], widths[i + 1], aggr, my) for i in range(num_layers))
        self.bns = torch.nn.ModuleList(torch.nn.BatchNorm1d(hidden).double() for _ in range(num_layers - 1))

    def forward(self, x, csr):
        for conv, bn in zip(self.convs[:-1], self.bns):
            x = bn(conv(x, csr))
        return self.convs[-1](x, csr)


# ---- the yardstick itself ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["max", "min"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_scatter_reduce(mode, seed):
    g = torch.Generator().manual_seed(seed)
    n, e, d = 90, 700, 5
    ei = torch.randint(0, n - 10, (2, e), generator=g)  # the last ten nodes have no in-edge (and no out-edge)
    x = torch.randn(n, d, generator=g, dtype=torch.float64, requires_grad=True)
    rowptr, col = host_csr(ei, n)
    out, arg = ref_extremum(rowptr, col, x, mode)
    xs = x.detach().clone().requires_grad_(True)
    want = torch.zeros(n, d, dtype=torch.float64).scatter_reduce(
        0, ei[1][:, None].expand(-1, d), xs[ei[0]], "amax" if mode == "max" else "amin", include_self=False)
    assert torch.equal(out, want)
    assert (arg[n - 10:] == -1).all() and (out[n - 10:] == 0).all() and (arg[:n - 10] >= -1).all()
    # continuous features: ties only between duplicate edges (same source), so both gradients send each target's whole
    # cotangent to its one extremal source. A source's gradient is a float64 sum over a handful of targets taken in two
    # different orders: equal to a few ulp of values of order 1-10
    cot = torch.randn(n, d, generator=g, dtype=torch.float64)
    (out * cot).sum().backward()
    (want * cot).sum().backward()
    assert (x.grad != 0).any() and torch.allclose(x.grad, xs.grad, rtol=0, atol=1e-13)


def test_restatement_takes_the_first_of_tied_slots():
    rowptr = torch.tensor([0, 4, 4, 6])
    col = torch.tensor([2, 0, 1, 0, 1, 1])
    x = torch.tensor([[1.0, 0.0], [1.0, 5.0], [0.0, 5.0]], dtype=torch.float64, requires_grad=True)
    out, arg = ref_extremum(rowptr, col, x, "max")
    assert arg.tolist() == [[1, 0], [-1, -1], [4, 4]]
    assert out.tolist() == [[1.0, 5.0], [0.0, 0.0], [1.0, 5.0]]
    out.sum().backward()  # a duplicate edge (slots 4, 5: both from node 1) counts once
    assert x.grad.tolist() == [[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]
    assert first_extremal_slot(rowptr, col, x.detach(), "min").tolist() == [[0, 1], [-1, -1], [4, 4]]


# ---- C ABI -------------------------------------------------------------------------------------------------------------

def test_header_exports_and_argument_checks():
    from rgb_experiment_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "rgbx_hip.h")).read()
    declared = set(re.findall(r"\b(rgbx_[a-z0-9_]+)\s*\(", header))
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.rgbx_version() == 501
    doc = header[header.index("Max / min neighbourhood aggregation"):header.index("rgbx_spmm_csr_extremum_f32(")]
    assert "inputs are finite" in doc.lower()
    assert lib.rgbx_spmm_csr_extremum_supported(128) == 1 and lib.rgbx_spmm_csr_extremum_supported(7) == 0
    assert lib.rgbx_spmm_csr_extremum_supported(260) == 0 and lib.rgbx_spmm_csr_extremum_supported(0) == 0
    p = 4096  # non-null, 16-byte aligned, never dereferenced: every call below fails before a launch
    fwd = lambda **k: lib.rgbx_spmm_csr_extremum_f32(k.get("rowptr", p), p, k.get("x", p), k.get("ldx", 8), k.get("out", p + 4096),
                                                     8, k.get("arg", p), k.get("N", 5), k.get("d", 8), k.get("mode", 0), None, None)
    assert fwd(rowptr=0) == -1 and fwd(x=0) == -1 and fwd(out=0) == -1 and fwd(N=-1) == -1 and fwd(mode=2) == -1
    assert fwd(ldx=4) == -1 and fwd(out=p) == -1  # leading dimension < d; out aliases x
    assert fwd(d=6) == -5 and fwd(d=260) == -5
    assert fwd(x=p + 4) == -3 and fwd(arg=p + 8) == -3
    assert fwd(N=0) == 0 and fwd(N=0, arg=0) == 0  # nothing to do; arg is optional
    bwd = lambda **k: lib.rgbx_extremum_bwd_f32(k.get("rowptr", p), p, k.get("t2f", p), k.get("gout", p), k.get("ldg", 8),
                                                k.get("arg", p), k.get("gx", p + 4096), 8, k.get("N", 5), k.get("d", 8), None, None)
    assert bwd(rowptr=0) == -1 and bwd(t2f=0) == -1 and bwd(gout=0) == -1 and bwd(arg=0) == -1 and bwd(gx=0) == -1
    assert bwd(N=-1) == -1 and bwd(ldg=4) == -1 and bwd(gx=p) == -1
    assert bwd(d=6) == -5 and bwd(gout=p + 4) == -3 and bwd(N=0) == 0


# ---- layers, models, experiment() -------------------------------------------------------------------------------------

def test_layers_and_models_take_the_keyword():
    from rgb_experiment_amd.models import GraphSAGE, GraphSAGE2
    from rgb_experiment_amd.nn import MySAGEConv, SAGEConv
    for aggr in AGGRS:
        want = "add" if aggr == "sum" else aggr
        assert SAGEConv(8, 4, aggr=aggr).aggr == want
        assert MySAGEConv(8, 4, aggr=aggr).aggr == want and MySAGEConv(8, 4, add_self_loops=False, aggr=aggr).aggr == want
        for cls in (GraphSAGE, GraphSAGE2):
            model = cls(num_layers=3, hidden_unit=8, input_dim=6, output_dim=3, dropout_rate=0.5, aggr=aggr)
            assert [c.aggr for c in model.convs] == [want] * 3
    assert SAGEConv(8, 4).aggr == "mean" and MySAGEConv(8, 4).aggr == "mean"
    for bad in ("median", "MAX", None, "lstm"):
        for make in (lambda a: SAGEConv(8, 4, aggr=a), lambda a: MySAGEConv(8, 4, aggr=a),
                     lambda a: GraphSAGE(2, 8, 6, 3, 0.5, aggr=a), lambda a: GraphSAGE2(2, 8, 6, 3, 0.5, aggr=a)):
            with pytest.raises(ValueError, match="aggr"):
                make(bad)


FORMS = ("accepts_ce", "accepts_ce_pair", "folds_post_affine", "emits_colsums")


def test_mean_instances_are_what_they_were():
    from rgb_experiment_amd.models._stack import _layer_maps
    from rgb_experiment_amd.nn import MySAGEConv, SAGEConv
    for cls, keys in ((SAGEConv, ["lin_l.weight", "lin_l.bias", "lin_r.weight"]),
                      (MySAGEConv, ["lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias"])):
        for conv in (cls(8, 4), cls(8, 4, aggr="mean")):
            assert list(conv.state_dict()) == keys
            for form in FORMS:  # class attributes, untouched on the instance
                assert getattr(conv, form) is True and getattr(cls, form) is True and form not in vars(conv)
            assert _layer_maps(conv) is not None
        assert list(cls(8, 4, aggr="max").state_dict()) == keys


@pytest.mark.parametrize("aggr", ["max", "min", "add", "sum"])
def test_other_aggregators_report_no_sum_only_form(aggr):
    from rgb_experiment_amd.models import GraphSAGE, GraphSAGE2
    from rgb_experiment_amd.models._stack import _layer_maps
    from rgb_experiment_amd.nn import MySAGEConv, SAGEConv
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1, 2], [1, 2, 0]])
    for conv in (SAGEConv(4, 8, aggr=aggr), MySAGEConv(4, 8, aggr=aggr), MySAGEConv(4, 8, add_self_loops=False, aggr=aggr)):
        for form in FORMS:
            assert getattr(conv, form) is False and getattr(type(conv), form) is True
        assert conv.eval_operands() is None
        assert conv.aggregate_input(x, ei) is None
        assert conv.forward_folded(x, ei, (None, None, None)) is None
        assert _layer_maps(conv) is None
    for cls in (GraphSAGE, GraphSAGE2):
        model = cls(num_layers=2, hidden_unit=16, input_dim=4, output_dim=3, dropout_rate=0.5, aggr=aggr).eval()
        assert model._collapsed_operands() is None
        assert model._eval_operands() == [None, None]


def test_cpu_tensors_are_refused():
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.nn import MySAGEConv, SAGEConv
    for fn in (ops.propagate_max, ops.propagate_min):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(torch.randn(5, 4), None)
    with pytest.raises(ValueError, match="max"):
        ops.spmm_extremum_raw(None, torch.randn(5, 4), "median", True)
    ei = torch.tensor([[0, 1], [1, 2]])
    for conv in (SAGEConv(4, 3, aggr="max"), MySAGEConv(4, 3, aggr="min"), SAGEConv(4, 3, aggr="add")):
        with pytest.raises(RuntimeError, match="no CPU fallback|No CPU fallback|HIP"):
            conv(torch.randn(5, 4), ei)


def test_a_partitioned_graph_is_refused():
    from rgb_experiment_amd import ops

    class Partitioned:
        is_distributed = True

    for fn in (ops.propagate_max, ops.propagate_min):
        with pytest.raises(NotImplementedError, match="partitioned"):
            fn(torch.randn(5, 4), Partitioned())


def test_experiment_refuses_the_distributed_route():
    from rgb_experiment_amd import experiment
    from rgb_experiment_amd.data import Data
    g = torch.Generator().manual_seed(5)
    n = 60
    data = Data(x=torch.randn(n, 8, generator=g), y=torch.randint(0, 3, (n,), generator=g),
                edge_index=torch.randint(0, n, (2, 300), generator=g))
    init = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.5, "aggr": "max"}
    for name in ("graphsage", "graphsage2"):
        with pytest.raises(NotImplementedError, match="partitioned"):
            experiment(init, specify_data=True, data=data, remake_data_mask=True, epoch=2, print_print=False,
                       need_to_reappear=True, use_cpu=True, model_name=name, distributed=True)
