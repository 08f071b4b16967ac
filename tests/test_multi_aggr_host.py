"""std / var and one-pass multi-aggregation on the host: the float64 restatement that tests/test_gpu_multi_aggr.py measures
the kernels against (pinned here to torch.scatter_reduce, torch.var and a hand-derived answer), the `aggr` keyword of the
SAGE layers and models as a string ('std', 'var') and as a list, every refusal, and the C ABI's argument checks (before any
launch). No GPU needed.

Semantics restated (PyG >= 2.1; a target row i with n slots p, v_p = x[col[p], c]):
  sum = sum_p v_p, mean = sum / max(n, 1), var = mean(v^2) - mean(v)^2 (biased, not clamped),
  std = s where s = sqrt(max(var, 1e-5)) and s > sqrt(1e-5), else 0; max / min / arg as tests/test_extremum_host.py.
A row without slots gives 0 everywhere."""
import math
import os
import re

import pytest
import torch

from test_extremum_host import FORMS, host_csr, ref_extremum, ref_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STATS = ("sum", "mean", "var", "std", "max", "min")
FOUR = ("mean", "max", "min", "std")
NEW_ENTRIES = ("rgbx_spmm_csr_multi_supported", "rgbx_spmm_csr_multi_partial_words", "rgbx_spmm_csr_multi_f32",
               "rgbx_multi_bwd_f32")
STD_FLOOR = 1e-5


# ---- the float64 restatement -------------------------------------------------------------------------------------------

def ref_var(rowptr, col, x):
    cnt = (rowptr[1:] - rowptr[:-1]).clamp(min=1).to(x.dtype)[:, None]
    mean = ref_sum(rowptr, col, x) / cnt
    return ref_sum(rowptr, col, x * x) / cnt - mean * mean


def _sqrt_floor(like):
    """sqrt(1e-5) from the SAME sqrt that produced the clamped values (torch's may differ from libm's in the last bit)."""
    return torch.sqrt(torch.tensor(STD_FLOOR, dtype=like.dtype))


def ref_stat(rowptr, col, x, name):
    """One statistic [n, d] of every row's neighbourhood, differentiable in x."""
    name = "sum" if name == "add" else name
    if name in ("max", "min"):
        return ref_extremum(rowptr, col, x, name)[0]
    if name in ("sum", "mean"):
        out = ref_sum(rowptr, col, x)
        return out if name == "sum" else out / (rowptr[1:] - rowptr[:-1]).clamp(min=1).to(x.dtype)[:, None]
    var = ref_var(rowptr, col, x)
    if name == "var":
        return var
    assert name == "std", name
    s = torch.sqrt(var.clamp(min=STD_FLOOR))
    return torch.where(s <= _sqrt_floor(s), torch.zeros_like(s), s)


def ref_multi(rowptr, col, x, names):
    return torch.cat([ref_stat(rowptr, col, x, a) for a in names], dim=1)


def std_band(rowptr, col, x):
    """bool [n, d]: the float64 variance lies in [0.5e-5, 2e-5] — around the kink of std, where a rounding decides between 0
    and sqrt(1e-5); such elements are left out of std comparisons."""
    var = ref_var(rowptr, col, x.detach().double())
    return (var >= 0.5 * STD_FLOOR) & (var <= 2 * STD_FLOOR)


class RefConv(torch.nn.Module):
    """float64 twin of nn.SAGEConv (my=False: aggregate x — one statistic or the concatenation of a list — then
    lin_l(agg) + lin_r(x)) and of nn.MySAGEConv (my=True: lin_l, lin_r, aggregate x_l, += x_r) over (rowptr, col)."""

    def __init__(self, cin, cout, aggr, my):
        super().__init__()
        self.names, self.my = ((aggr,) if isinstance(aggr, str) else tuple(aggr)), my
        assert not (my and len(self.names) > 1)
        self.lin_l = torch.nn.Linear(cin * (1 if my else len(self.names)), cout, bias=True).double()
        self.lin_r = torch.nn.Linear(cin, cout, bias=my).double()

    def forward(self, x, csr):
        if self.my:
            return ref_multi(csr[0], csr[1], self.lin_l(x), self.names) + self.lin_r(x)
        return self.lin_l(ref_multi(csr[0], csr[1], x, self.names)) + self.lin_r(x)


class RefStack(torch.nn.Module):
    """(conv -> BatchNorm1d) x (L-1), conv in float64 with the state_dict keys of GraphSAGE / GraphSAGE2."""

    def __init__(self, num_layers, hidden, cin, cout, aggr, my):
        super().__init__()
        widths = [cin] + [hidden] * (num_layers - 1) + [cout]
        self.convs = torch.nn.ModuleList(RefConv(widths[i], widths[i + 1], aggr, my) for i in range(num_layers))
        self.bns = torch.nn.ModuleList(torch.nn.BatchNorm1d(hidden).double() for _ in range(num_layers - 1))

    def forward(self, x, csr):
        for conv, bn in zip(self.convs[:-1], self.bns):
            x = bn(conv(x, csr))
        return self.convs[-1](x, csr)


# ---- the yardstick itself ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_scatter_reduce_and_torch_var(seed):
    g = torch.Generator().manual_seed(seed)
    n, e, d = 90, 700, 5
    ei = torch.randint(0, n - 10, (2, e), generator=g)  # the last ten nodes have no in-edge
    x = torch.randn(n, d, generator=g, dtype=torch.float64)
    rowptr, col = host_csr(ei, n)
    idx = ei[1][:, None].expand(-1, d)
    zeros = torch.zeros(n, d, dtype=torch.float64)
    want_sum = zeros.scatter_reduce(0, idx, x[ei[0]], "sum", include_self=False)
    want_mean = zeros.scatter_reduce(0, idx, x[ei[0]], "mean", include_self=False)
    assert torch.allclose(ref_stat(rowptr, col, x, "sum"), want_sum, rtol=0, atol=1e-12)
    assert torch.allclose(ref_stat(rowptr, col, x, "add"), want_sum, rtol=0, atol=1e-12)
    assert torch.allclose(ref_stat(rowptr, col, x, "mean"), want_mean, rtol=0, atol=1e-12)
    assert torch.equal(ref_stat(rowptr, col, x, "max"), zeros.scatter_reduce(0, idx, x[ei[0]], "amax", include_self=False))
    assert torch.equal(ref_stat(rowptr, col, x, "min"), zeros.scatter_reduce(0, idx, x[ei[0]], "amin", include_self=False))
    var, std = ref_stat(rowptr, col, x, "var"), ref_stat(rowptr, col, x, "std")
    for i in range(n):
        seg = x[ei[0][ei[1] == i]]
        if seg.size(0) == 0:
            assert (var[i] == 0).all() and (std[i] == 0).all()
            continue
        v = torch.var(seg, dim=0, unbiased=False)
        assert torch.allclose(var[i], v, rtol=0, atol=1e-12)
        s = torch.sqrt(v.clamp(min=STD_FLOOR))
        assert torch.allclose(std[i], torch.where(s <= _sqrt_floor(s), torch.zeros_like(s), s), rtol=0, atol=1e-12)
    out = ref_multi(rowptr, col, x, FOUR)
    assert out.shape == (n, 4 * d) and torch.equal(out[:, 3 * d:], std)
    assert torch.equal(out[:, :d], ref_stat(rowptr, col, x, "mean")) and torch.equal(out[:, d:2 * d], ref_stat(rowptr, col, x, "max"))


def test_known_answer_on_five_edges():
    """Edges 0->1, 2->1, 2->1 (a duplicate), 3->2, 3->0; node 3 has no in-edge. Slots: row 0 = [3], row 1 = [0, 2, 2],
    row 2 = [3], row 3 = []. Column 0 of row 1 gathers 1, 4, 4: sum 9, mean 3, var (1 + 16 + 16)/3 - 9 = 2; column 1
    gathers 3, 3, 3: var 0, so std 0. Rows 0 and 2 have degree 1: var = std = 0."""
    ei = torch.tensor([[0, 2, 2, 3, 3], [1, 1, 1, 2, 0]])
    x = torch.tensor([[1.0, 3.0], [2.0, 5.0], [4.0, 3.0], [8.0, 7.0]], dtype=torch.float64, requires_grad=True)
    rowptr, col = host_csr(ei, 4)
    assert rowptr.tolist() == [0, 1, 4, 5, 5] and col.tolist() == [3, 0, 2, 2, 3]
    st = {a: ref_stat(rowptr, col, x, a) for a in STATS}
    assert st["sum"].tolist() == [[8.0, 7.0], [9.0, 9.0], [8.0, 7.0], [0.0, 0.0]]
    assert st["mean"].tolist() == [[8.0, 7.0], [3.0, 3.0], [8.0, 7.0], [0.0, 0.0]]
    assert st["var"].tolist() == [[0.0, 0.0], [2.0, 0.0], [0.0, 0.0], [0.0, 0.0]]
    assert abs(st["std"][1, 0].item() - math.sqrt(2.0)) < 1e-15 and (st["std"].flatten()[[0, 1, 3, 4, 5, 6, 7]] == 0).all()
    assert st["max"].tolist() == [[8.0, 7.0], [4.0, 3.0], [8.0, 7.0], [0.0, 0.0]]
    assert st["min"].tolist() == [[8.0, 7.0], [1.0, 3.0], [8.0, 7.0], [0.0, 0.0]]
    assert ref_extremum(rowptr, col, x, "max")[1].tolist() == [[0, 0], [2, 1], [4, 4], [-1, -1]]  # lowest slot on ties
    assert ref_extremum(rowptr, col, x, "min")[1].tolist() == [[0, 0], [1, 1], [4, 4], [-1, -1]]
    # d std / d x_j = (x_j - mean) / (n std) per slot: row 1, column 0: (1 - 3) / (3 sqrt 2) once for node 0, (4 - 3) /
    # (3 sqrt 2) twice for node 2; 0 wherever the clamp / mask is active (every other element)
    (gs,) = torch.autograd.grad(st["std"].sum(), x, retain_graph=True)
    r = 1.0 / (3.0 * math.sqrt(2.0))
    assert torch.allclose(gs, torch.tensor([[-2 * r, 0.0], [0.0, 0.0], [2 * r, 0.0], [0.0, 0.0]], dtype=torch.float64), atol=1e-15)
    (gv,) = torch.autograd.grad(st["var"].sum(), x)  # 2 (x_j - mean) / n per slot, no clamp: zero only where x_j = mean
    assert torch.allclose(gv, torch.tensor([[-4 / 3, 0.0], [0.0, 0.0], [4 / 3, 0.0], [0.0, 0.0]], dtype=torch.float64), atol=1e-15)


def _f32_std(rowptr, col, x, shifted):
    """std in float32 arithmetic: sum x^2 / n - (sum x / n)^2 as it stands, or on deviations from the row's first slot."""
    n = rowptr.numel() - 1
    deg = rowptr[1:] - rowptr[:-1]
    row = torch.repeat_interleave(torch.arange(n), deg)
    v = x[col]
    if shifted:
        first = x[col[rowptr[:-1].clamp(max=col.numel() - 1)]]
        v = v - first[row]
    cnt = deg.clamp(min=1).float()[:, None]
    z = torch.zeros(n, x.size(1))
    m = z.index_add(0, row, v) / cnt
    var = z.index_add(0, row, v * v) / cnt - m * m
    return torch.where(var > STD_FLOOR, var.clamp(min=0).sqrt(), torch.zeros_like(var))


def test_offset_features_need_the_shifted_second_moment():
    """x = 50 + 0.05 randn: the bar tests/test_gpu_multi_aggr.py holds std to (1e-4 |ref|max, no floor of 1) is met by
    float32 sums of deviations from a shift inside the data and missed by float32 sum(x^2)/n - (sum(x)/n)^2."""
    g = torch.Generator().manual_seed(3)
    n = 700
    ei = torch.randint(0, n, (2, 6000), generator=g)
    x = 50 + 0.05 * torch.randn(n, 64, generator=g)
    rowptr, col = host_csr(ei, n)
    ref = ref_stat(rowptr, col, x.double(), "std")
    keep = ~std_band(rowptr, col, x)
    bar = 1e-4 * ref.abs().max().item()
    err = lambda got: ((got.double() - ref).abs() * keep).max().item()
    print(f"bar {bar:.3e}, shifted {err(_f32_std(rowptr, col, x, True)):.3e}, naive {err(_f32_std(rowptr, col, x, False)):.3e}")
    assert err(_f32_std(rowptr, col, x, True)) < bar < err(_f32_std(rowptr, col, x, False))


# ---- C ABI -------------------------------------------------------------------------------------------------------------

def test_header_exports_and_argument_checks():
    import ctypes
    from rgb_experiment_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "rgbx_hip.h")).read()
    declared = set(re.findall(r"\b(rgbx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.rgbx_version() == 501
    doc = header[header.index("one-pass multi-aggregation"):header.index("int rgbx_spmm_csr_multi_supported(")]
    assert "inputs are finite" in doc.lower() and "rgbx_multi_out_t" in doc
    ok = lib.rgbx_spmm_csr_multi_supported
    assert ok(128) == 1 and ok(4) == 1 and ok(256) == 1 and ok(7) == 0 and ok(260) == 0 and ok(0) == 0
    words = ctypes.c_int64(-1)
    pw = lib.rgbx_spmm_csr_multi_partial_words
    assert pw(10, 64, 2 | 8 | 16 | 32, ctypes.byref(words)) == 0 and words.value == 10 * 64 * (1 + 3 + 2 + 2)
    assert pw(10, 64, 1 | 2, ctypes.byref(words)) == 0 and words.value == 10 * 64      # sum and mean share the sum
    assert pw(10, 64, 4, ctypes.byref(words)) == 0 and words.value == 10 * 64 * 3      # shifted sum, squares, shift
    assert pw(10, 64, 0, ctypes.byref(words)) == -1 and pw(10, 64, 64, ctypes.byref(words)) == -1
    assert pw(10, 64, 2, None) == -1 and pw(-1, 64, 2, ctypes.byref(words)) == -1

    p = 4096  # non-null, 16-byte aligned, never dereferenced: every call below fails before a launch
    fields = ("sum", "mean", "var", "std", "max", "argmax", "min", "argmin")

    def fwd(outs=("mean", "std", "max", "argmax"), rowptr=p, x=p, ldx=8, N=5, d=8, ld=8, null_out=False, **ptrs):
        o = _lib.MultiOut()
        for i, f in enumerate(fields):
            if f in outs:
                setattr(o, f, ptrs.get(f, p + 4096 * (i + 1)))
                setattr(o, "ld_" + f, ld)
        return lib.rgbx_spmm_csr_multi_f32(rowptr, p, x, ldx, None if null_out else ctypes.byref(o), N, d, None, None)

    assert fwd(rowptr=0) == -1 and fwd(x=0) == -1 and fwd(null_out=True) == -1 and fwd(N=-1) == -1
    assert fwd(outs=()) == -1 and b"no statistic" in lib.rgbx_last_error_string()
    assert fwd(outs=("mean", "argmax")) == -1 and fwd(outs=("argmin",)) == -1    # an arg without its extremum
    assert fwd(ldx=4) == -1 and fwd(ld=4) == -1 and fwd(mean=p) == -1 and fwd(argmax=p) == -1   # ld < d; aliases x
    assert fwd(d=6) == -5 and fwd(d=260, ld=260, ldx=260) == -5
    assert fwd(x=p + 4) == -3 and fwd(std=p + 8) == -3 and fwd(argmax=p + 4) == -3 and fwd(ld=10) == -3 and fwd(ldx=10) == -3
    assert fwd(N=0) == 0 and fwd(N=0, outs=("max",)) == 0 and fwd(N=0, outs=STATS) == 0   # nothing to do; args optional

    gfields = ("a", "b", "x", "gmax", "argmax", "gmin", "argmin")

    def bwd(terms=gfields, rowptr=p, t2f=p, gx=p + 4096 * 9, ldgx=8, N=5, d=8, ld=8, null_terms=False, **ptrs):
        t = _lib.MultiGrad()
        for i, f in enumerate(gfields):
            if f in terms:
                setattr(t, f, ptrs.get(f, p + 4096 * (i + 1)))
                setattr(t, "ld_" + f, ld)
        return lib.rgbx_multi_bwd_f32(rowptr, p, t2f, None if null_terms else ctypes.byref(t), gx, ldgx, N, d, None, None)

    assert bwd(rowptr=0) == -1 and bwd(null_terms=True) == -1 and bwd(gx=0) == -1 and bwd(N=-1) == -1
    assert bwd(terms=()) == -1 and bwd(terms=("x",)) == -1                           # no term
    assert bwd(terms=("gmax",)) == -1 and bwd(terms=("a", "argmin")) == -1             # cotangent and arg go together
    assert bwd(t2f=0) == -1 and bwd(terms=("a", "b", "x"), t2f=0, N=0) == 0            # t2f only with an extremum term
    assert bwd(terms=("a", "b")) == -1                                                 # b needs x
    assert bwd(ldgx=4) == -1 and bwd(ld=4) == -1 and bwd(gx=p + 4096) == -1            # ld < d; gx aliases a
    assert bwd(d=6) == -5 and bwd(d=260, ld=260, ldgx=260) == -5
    assert bwd(a=p + 4) == -3 and bwd(argmin=p + 8) == -3 and bwd(gx=p + 4) == -3 and bwd(ld=10) == -3
    assert bwd(N=0) == 0 and bwd(N=0, terms=("a",)) == 0 and bwd(N=0, terms=("gmin", "argmin")) == 0


# ---- layers, models, experiment() -------------------------------------------------------------------------------------

def test_strings_std_and_var_are_accepted_everywhere():
    from rgb_experiment_amd.models import GraphSAGE, GraphSAGE2
    from rgb_experiment_amd.nn import MySAGEConv, SAGEConv
    from rgb_experiment_amd.nn.conv import AGGRS
    assert AGGRS["std"] == "std" and AGGRS["var"] == "var"
    for aggr in ("std", "var"):
        assert SAGEConv(8, 4, aggr=aggr).aggr == aggr
        assert MySAGEConv(8, 4, aggr=aggr).aggr == aggr and MySAGEConv(8, 4, add_self_loops=False, aggr=aggr).aggr == aggr
        assert SAGEConv(8, 4, aggr=aggr).lin_l.weight.shape == (4, 8)
        for cls in (GraphSAGE, GraphSAGE2):
            model = cls(num_layers=3, hidden_unit=8, input_dim=6, output_dim=3, dropout_rate=0.5, aggr=aggr)
            assert [c.aggr for c in model.convs] == [aggr] * 3
    for bad in ("median", "MAX", None, "lstm"):
        for make in (lambda a: SAGEConv(8, 4, aggr=a), lambda a: MySAGEConv(8, 4, aggr=a),
                     lambda a: GraphSAGE(2, 8, 6, 3, 0.5, aggr=a), lambda a: GraphSAGE2(2, 8, 6, 3, 0.5, aggr=a)):
            with pytest.raises(ValueError, match="aggr"):
                make(bad)


def test_lists_of_aggregators():
    from rgb_experiment_amd.models import GraphSAGE, GraphSAGE2
    from rgb_experiment_amd.nn import MySAGEConv, SAGEConv
    keys = ["lin_l.weight", "lin_l.bias", "lin_r.weight"]
    for aggr, want in ((["mean", "max", "min", "std"], FOUR), (("sum", "var"), ("add", "var")), (["mean"], ("mean",)),
                       (["add", "std", "max"], ("add", "std", "max"))):
        conv = SAGEConv(8, 4, aggr=aggr)
        assert conv.aggr == want and isinstance(conv.aggr, tuple)
        assert conv.lin_l.weight.shape == (4, len(want) * 8) and conv.lin_r.weight.shape == (4, 8)
        assert list(conv.state_dict()) == keys
    model = GraphSAGE2(num_layers=3, hidden_unit=8, input_dim=6, output_dim=3, dropout_rate=0.5, aggr=list(FOUR))
    assert [c.aggr for c in model.convs] == [FOUR] * 3
    assert [tuple(c.lin_l.weight.shape) for c in model.convs] == [(8, 24), (8, 32), (3, 32)]
    plain = GraphSAGE2(num_layers=3, hidden_unit=8, input_dim=6, output_dim=3, dropout_rate=0.5)
    assert list(model.state_dict()) == list(plain.state_dict())
    for bad in ([], (), ["mean", "mean"], ["sum", "add"], ["mean", "median"], ["mean", None], [["mean"]], ["MAX"]):
        for make in (lambda a: SAGEConv(8, 4, aggr=a), lambda a: GraphSAGE2(2, 8, 6, 3, 0.5, aggr=a)):
            with pytest.raises(ValueError, match="aggr"):
                make(bad)
    # the reference's layer has no projection for a concatenation
    for make in (lambda a: MySAGEConv(8, 4, aggr=a), lambda a: MySAGEConv(8, 4, add_self_loops=False, aggr=a),
                 lambda a: GraphSAGE(2, 8, 6, 3, 0.5, aggr=a)):
        for aggr in (list(FOUR), ("mean",), []):
            with pytest.raises(ValueError, match="aggr"):
                make(aggr)


def test_mean_instances_are_what_they_were_beside_a_std_instance():
    from rgb_experiment_amd.models._stack import _layer_maps
    from rgb_experiment_amd.nn import MySAGEConv, SAGEConv
    for cls, keys in ((SAGEConv, ["lin_l.weight", "lin_l.bias", "lin_r.weight"]),
                      (MySAGEConv, ["lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias"])):
        other = [cls(8, 4, aggr="std"), cls(8, 4, aggr="var")] + ([cls(8, 4, aggr=["mean", "std"])] if cls is SAGEConv else [])
        for conv in (cls(8, 4), cls(8, 4, aggr="mean")):
            assert conv.aggr == "mean" and list(conv.state_dict()) == keys
            for form in FORMS:  # class attributes, untouched on the instance
                assert getattr(conv, form) is True and getattr(cls, form) is True and form not in vars(conv)
            assert _layer_maps(conv) is not None
            assert conv.lin_l.weight.shape == (4, 8)
        for conv in other:
            assert list(conv.state_dict()) == keys


@pytest.mark.parametrize("aggr", ["std", "var", ["mean", "max", "min", "std"], ["mean"]])
def test_new_aggregators_report_no_sum_only_form(aggr):
    from rgb_experiment_amd.models import GraphSAGE, GraphSAGE2
    from rgb_experiment_amd.models._stack import _layer_maps
    from rgb_experiment_amd.nn import MySAGEConv, SAGEConv
    x, ei = torch.randn(6, 4), torch.tensor([[0, 1, 2], [1, 2, 0]])
    convs = [SAGEConv(4, 8, aggr=aggr)]
    if isinstance(aggr, str):
        convs += [MySAGEConv(4, 8, aggr=aggr), MySAGEConv(4, 8, add_self_loops=False, aggr=aggr)]
    for conv in convs:
        for form in FORMS:
            assert getattr(conv, form) is False and getattr(type(conv), form) is True
        assert conv.eval_operands() is None
        assert conv.aggregate_input(x, ei) is None
        assert conv.forward_folded(x, ei, (None, None, None)) is None
        assert _layer_maps(conv) is None
    for cls in (GraphSAGE2,) + ((GraphSAGE,) if isinstance(aggr, str) else ()):
        model = cls(num_layers=2, hidden_unit=16, input_dim=4, output_dim=3, dropout_rate=0.5, aggr=aggr).eval()
        assert model._collapsed_operands() is None
        assert model._eval_operands() == [None, None]


def test_cpu_tensors_are_refused():
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.nn import MySAGEConv, SAGEConv
    for fn in (ops.propagate_std, ops.propagate_var, lambda x, g: ops.propagate_multi(x, g, FOUR),
               lambda x, g: ops.spmm_multi_raw(g, x, FOUR, True), lambda x, g: ops.multi_bwd_raw(g, a=x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(torch.randn(5, 4), None)
    for bad in ("median", [], ["mean", "mean"], ["mean", 3]):
        with pytest.raises(ValueError, match="aggr"):
            ops.propagate_multi(torch.randn(5, 4), None, bad)
    ei = torch.tensor([[0, 1], [1, 2]])
    for conv in (SAGEConv(4, 3, aggr="std"), MySAGEConv(4, 3, aggr="var"), SAGEConv(4, 3, aggr=["mean", "std"])):
        with pytest.raises(RuntimeError, match="no CPU fallback|No CPU fallback|HIP"):
            conv(torch.randn(5, 4), ei)


def test_a_partitioned_graph_is_refused():
    from rgb_experiment_amd import ops

    class Partitioned:
        is_distributed = True

    for fn in (ops.propagate_std, ops.propagate_var, lambda x, g: ops.propagate_multi(x, g, FOUR)):
        with pytest.raises(NotImplementedError, match="partitioned"):
            fn(torch.randn(5, 4), Partitioned())


def test_experiment_refuses_the_distributed_route():
    from rgb_experiment_amd import experiment
    from rgb_experiment_amd.data import Data
    g = torch.Generator().manual_seed(5)
    n = 60
    data = Data(x=torch.randn(n, 8, generator=g), y=torch.randint(0, 3, (n,), generator=g),
                edge_index=torch.randint(0, n, (2, 300), generator=g))
    for name, aggr in (("graphsage", "std"), ("graphsage2", "var"), ("graphsage2", list(FOUR))):
        init = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.5, "aggr": aggr}
        with pytest.raises(NotImplementedError, match="partitioned"):
            experiment(init, specify_data=True, data=data, remake_data_mask=True, epoch=2, print_print=False,
                       need_to_reappear=True, use_cpu=True, model_name=name, distributed=True)
