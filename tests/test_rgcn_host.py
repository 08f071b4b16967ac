"""RGCNConv on the host: a float64 restatement of the layer, written PER RELATION WITH MASKS (for every relation r the
edges of that relation are selected, their messages x_j @ W_r summed per target and divided by their count), not with CSR
slots and slot weights as the product computes it; pinned by numbers derived by hand. Registry, module layout (PyG's
names, strict state_dict loading both ways), refusals, the use_edge_type keyword of experiment() and the C ABI of the new
entry points; and the case builders tests/test_gpu_rgcn.py feeds to the HIP kernels, with the checks that keep those
cases well-posed. No GPU needed.

Well-posedness. Everything here is linear in the inputs (no kink, no softmax), so what separates float32 from float64 is
summation error alone: every case is run through the restatement in float32 on the CPU with the edges and the relations
in REVERSED order and has to stay within a QUARTER (WELL_POSED_SHARE) of the GPU test's tolerances (forward 1e-4,
gradients 2e-4, times max(1, |ref|max)) of the float64 result. Inputs are exactly representable in float32. Seeds are
fixed; a case that does not satisfy this fails, it is never skipped."""
import copy
import functools
import inspect
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from rgb_experiment_amd.models import RGCN             # without the feature this file fails here, at import
from rgb_experiment_amd.nn import RGCNConv

import test_gine_host as G
from test_transformer_host import FWD_TOL, GRAD_TOL, LONG_ROW_SLOTS, WELL_POSED_SHARE, f32_exact, share_of_tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------

def aggregate(rows, n, src, dst, et, aggr="mean", reverse=False):
    """out [n, C] = sum over the relations r of AGG over the edges (src -> dst) of relation r, as given, of
    rows[r, src, :]; rows [R, n, C] holds the message row of every (relation, source). AGG is the mean per (target,
    relation) — the sum divided by the number of edges of relation r into the target, duplicates counted — or the sum
    with aggr="add". A (target, relation) pair without an edge contributes 0. `reverse`: relations and edges backwards."""
    R, _, C = rows.shape
    out = torch.zeros(n, C, dtype=rows.dtype)
    for r in (reversed(range(R)) if reverse else range(R)):
        mine = (et == r).nonzero(as_tuple=True)[0]
        if reverse:
            mine = mine.flip(0)
        s, d = src[mine], dst[mine]
        tot = torch.zeros(n, C, dtype=rows.dtype).index_add(0, d, rows[r].index_select(0, s))
        if aggr == "mean":
            tot = tot / torch.bincount(d, minlength=n).clamp(min=1).to(rows.dtype)[:, None]
        elif aggr not in ("add", "sum"):
            raise ValueError(aggr)
        out = out + tot
    return out


def mix_rows(h, comp):
    """[R, n, C] from the basis products h [n, B * C] and comp [R, B]: the rows of x @ W_r, W_r = sum_b comp[r, b] V_b."""
    n, B = h.size(0), comp.size(1)
    return torch.einsum("rb,nbc->rnc", comp, h.view(n, B, -1))


def select_rows(h, R):
    """[R, n, C] from h [n, R * C] = x @ [W_0 | ... | W_{R-1}]."""
    return h.view(h.size(0), R, -1).permute(1, 0, 2)


class RefRGCNConv(nn.Module):
    """float64 restatement of RGCNConv with PyG's parameter names and shapes: weight [num_bases or R, in, out], comp
    [R, num_bases] only with num_bases, root [in, out] with root_weight, bias [out]."""

    def __init__(self, in_channels, out_channels, num_relations, num_bases=None, aggr="mean", root_weight=True,
                 bias=True):
        super().__init__()
        self.R, self.B, self.aggr = num_relations, num_bases, aggr
        f64 = lambda *shape: nn.Parameter(torch.zeros(*shape, dtype=torch.float64))
        self.weight = f64(num_bases or num_relations, in_channels, out_channels)
        self.comp = f64(num_relations, num_bases) if num_bases is not None else None
        self.root = f64(in_channels, out_channels) if root_weight else None
        self.bias = f64(out_channels) if bias else None

    def forward(self, x, ei, et, reverse=False):
        W = self.weight
        if self.comp is not None:
            W = (self.comp @ W.reshape(self.B, -1)).view(self.R, W.size(1), W.size(2))
        rows = torch.stack([x @ W[r] for r in range(self.R)])
        out = aggregate(rows, x.size(0), ei[0], ei[1], et, self.aggr, reverse)
        if self.root is not None:
            out = out + x @ self.root
        if self.bias is not None:
            out = out + self.bias
        return out


class RefRGCN(nn.Module):
    """models/rgcn.py in float64: num_layers RGCNConv layers, ReLU and dropout between them; the product's names."""

    def __init__(self, input_dim, output_dim, hidden_unit, num_layers, dropout_rate, num_relations, num_bases=None):
        super().__init__()
        self.dropout_rate = dropout_rate
        dims = [input_dim] + [hidden_unit] * (num_layers - 1) + [output_dim]
        self.convs = nn.ModuleList(RefRGCNConv(a, b, num_relations, num_bases) for a, b in zip(dims[:-1], dims[1:]))

    def forward(self, x, ei, et, reverse=False):
        for i, conv in enumerate(self.convs):
            x = conv(x, ei, et, reverse)
            if i + 1 < len(self.convs):
                x = F.dropout(F.relu(x), p=self.dropout_rate, training=self.training)
        return {"out": F.log_softmax(x, dim=1), "emb": x}


def randomize(module, seed):
    """Every parameter of a reference module set to fp32-exact N(0, 0.5) values."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(f32_exact(tuple(p.shape), g, 0.5))
    return module


# ---- graphs and edge types --------------------------------------------------------------------------------------------

graph_names = ("no_edges", "random", "powerlaw", "degrees") + G.SMALL_GRAPHS
RELATIONS = (1, 3, 7)
PLANTED_R = 4


@functools.lru_cache(maxsize=None)
def graph_of(name):
    """tests/test_gine_host.graph_of, plus `planted`: 6 nodes, 4 relations. Target 0: three in-edges, all of relation 0 (its
    mean is the plain mean). Target 1: three in-edges of relations 0, 1, 2 (all differ: every weight is 1). Target 2: the
    edge 4 -> 2 three times, twice with relation 1 (duplicates of one type) and once with relation 0. Node 3: a self-loop
    of relation 2. Nodes 4 and 5 have no in-edge; relation 3 owns no edge at all."""
    if name == "planted":
        return torch.tensor([[1, 2, 3, 0, 2, 3, 4, 4, 4, 3], [0, 0, 0, 1, 1, 1, 2, 2, 2, 3]]), 6
    return G.graph_of(name)


@functools.lru_cache(maxsize=None)
def edge_type_of(name, R):
    """int64 [E], seeded. With R > 1 the LAST relation owns no edge at all (its row of g_comp is an exact zero)."""
    if name == "planted":
        assert R == PLANTED_R
        return torch.tensor([0, 0, 0, 0, 1, 2, 1, 1, 0, 2])
    E = graph_of(name)[0].size(1)
    if R == 1:
        return torch.zeros(E, dtype=torch.int64)
    return torch.randint(0, R - 1, (E,), generator=torch.Generator().manual_seed(9000 + R))


@functools.lru_cache(maxsize=None)
def slots_of(name):
    if name == "planted":
        ei, n = graph_of(name)
        order = torch.argsort(ei[1], stable=True)
        rowptr = torch.zeros(n + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(torch.bincount(ei[1], minlength=n), 0)
        return ei[0], ei[1], rowptr, order
    return G.slots_of(name)


def slot_counts(name, R):
    """(etype, cnt) int64 [E] in forward CSR slot order: the relation of every slot and the number of slots of its row
    that share it, by torch's integer ops."""
    ei, n = graph_of(name)
    et = edge_type_of(name, R)
    key = ei[1] * R + et
    cnt = torch.bincount(key, minlength=n * R)[key]
    order = slots_of(name)[3]
    return et[order], cnt[order]


# ---- operator cases shared with tests/test_gpu_rgcn.py ----------------------------------------------------------------

BASES = [1, 2, 5, 8, 30]              # 30: the heads of a row in several chunks at every width above 2 floats
WIDTHS = [1, 4, 7, 16, 64, 66]        # vector widths 1 (1, 7), 2 (66) and 4 (4, 16, 64)
PADDED_WIDTH = 67                     # outside the layout: the layer pads it to 68
MIX_PAIRS = [(B, C) for B in BASES for C in WIDTHS]
# one pair per vector width, a multi-chunk head count and the smallest shape, for the sweeps over graphs and R
SWEEP_PAIRS = [(1, 1), (2, 7), (5, 66), (8, 64), (30, 16)]
MIX_CASES = ([(B, C, 3, "degrees", "mean") for B, C in MIX_PAIRS]
             + [(B, C, R, g, "mean") for B, C in SWEEP_PAIRS for R in RELATIONS for g in ("degrees", "powerlaw")
                if not (R == 3 and g == "degrees")]
             + [(2, 7, 3, g, "mean") for g in ("no_edges", "random") + G.SMALL_GRAPHS]
             + [(2, 4, PLANTED_R, "planted", "mean"), (2, 4, PLANTED_R, "planted", "add")]
             + [(5, 66, 3, "powerlaw", "add"), (8, 64, 7, "degrees", "sum")])
SELECT_WIDTHS = [5, 64]
SELECT_CASES = ([(C, R, g, "mean") for C in SELECT_WIDTHS for R in RELATIONS for g in ("degrees", "powerlaw")]
                + [(5, 3, g, "mean") for g in ("no_edges", "random") + G.SMALL_GRAPHS]
                + [(4, PLANTED_R, "planted", "mean"), (4, PLANTED_R, "planted", "add"), (64, 3, "powerlaw", "add")])
MIX_NAMES = ("forward", "g_h", "g_comp", "g_y0")
SELECT_NAMES = ("forward", "g_h", "g_y0")


@functools.lru_cache(maxsize=4)
def mix_case(B, C, R, graph_name):
    """h [n, B * C], comp [R, B], y0 [n, C] and the cotangent [n, C]: float64, fp32-exact, N(0, 1)."""
    _, n = graph_of(graph_name)
    g = torch.Generator().manual_seed(7000 + 100 * B + C + 7 * R)
    return f32_exact((n, B * C), g), f32_exact((R, B), g), f32_exact((n, C), g), f32_exact((n, C), g)


@functools.lru_cache(maxsize=4)
def select_case(C, R, graph_name):
    _, n = graph_of(graph_name)
    g = torch.Generator().manual_seed(8000 + C + 7 * R)
    return f32_exact((n, R * C), g), f32_exact((n, C), g), f32_exact((n, C), g)


def run_mix(case, R, graph_name, aggr, dtype=torch.float64, reverse=False):
    """The restatement on a mix case in `dtype`: (out, [g_h, g_comp, g_y0])."""
    ei, n = graph_of(graph_name)
    h, comp, y0 = (t.to(dtype).clone().requires_grad_(True) for t in case[:3])
    out = y0 + aggregate(mix_rows(h, comp), n, ei[0], ei[1], edge_type_of(graph_name, R), aggr, reverse)
    (out * case[3].to(dtype)).sum().backward()
    return out.detach(), [h.grad, comp.grad, y0.grad]


def run_select(case, R, graph_name, aggr, dtype=torch.float64, reverse=False):
    ei, n = graph_of(graph_name)
    h, y0 = (t.to(dtype).clone().requires_grad_(True) for t in case[:2])
    out = y0 + aggregate(select_rows(h, R), n, ei[0], ei[1], edge_type_of(graph_name, R), aggr, reverse)
    (out * case[2].to(dtype)).sum().backward()
    return out.detach(), [h.grad, y0.grad]


@functools.lru_cache(maxsize=4)
def mix_reference(B, C, R, graph_name, aggr):
    """The float64 result of a case, computed once and shared (read-only) by the host and the GPU tests."""
    return run_mix(mix_case(B, C, R, graph_name), R, graph_name, "add" if aggr == "sum" else aggr)


@functools.lru_cache(maxsize=4)
def select_reference(C, R, graph_name, aggr):
    return run_select(select_case(C, R, graph_name), R, graph_name, aggr)


def shares_of(got, want, names):
    out = {names[0]: share_of_tolerance(got[0], want[0], FWD_TOL)}
    for name, a, b in zip(names[1:], got[1], want[1]):
        assert a.shape == b.shape
        out[name] = share_of_tolerance(a, b, GRAD_TOL)
    return out


# ---- layer and model cases ----------------------------------------------------------------------------------------------

LAYER_N, LAYER_E, LAYER_F, LAYER_R = 80, 500, 6, 3
LAYER_CASES = {   # name -> (out_channels, layer keywords)
    "select": (7, dict()),
    "select_add": (7, dict(aggr="add")),
    "bases": (7, dict(num_bases=2)),
    "bases_padded": (PADDED_WIDTH, dict(num_bases=2)),
    "bases_sum_no_root": (16, dict(num_bases=5, aggr="sum", root_weight=False)),
    "bases_no_bias": (16, dict(num_bases=2, bias=False)),
    "bare": (5, dict(num_bases=2, root_weight=False, bias=False)),
    "too_many_bases": (4, dict(num_bases=65)),            # beyond the kernels' head count: W_r composed, select form
}


def layer_case(name):
    """(x float64 fp32-exact, edge_index, edge_type, reference layer with fp32-exact random parameters)."""
    from test_gpu_ggnn import rand_graph
    C, kw = LAYER_CASES[name]
    ei = rand_graph(LAYER_N, LAYER_E, 21, loops=5, dups=12)
    et = torch.randint(0, LAYER_R, (ei.size(1),), generator=torch.Generator().manual_seed(22))
    x = f32_exact((LAYER_N, LAYER_F), torch.Generator().manual_seed(23))
    return x, ei, et, randomize(RefRGCNConv(LAYER_F, C, LAYER_R, **kw), 24)


MODEL_SHAPE = dict(n=60, e=300, f=16, hidden=12, classes=5, layers=3, relations=4)


def model_case(num_bases=None):
    """(x, y, edge_index, edge_type, the product's model on the CPU, the reference holding the same parameters)."""
    from test_gpu_ggnn import rand_graph
    s = MODEL_SHAPE
    g = torch.Generator().manual_seed(31)
    ei = rand_graph(s["n"], s["e"], 32, loops=4, dups=6)
    et = torch.randint(0, s["relations"], (ei.size(1),), generator=g)
    x, y = f32_exact((s["n"], s["f"]), g), torch.randint(0, s["classes"], (s["n"],), generator=g)
    ref = randomize(RefRGCN(s["f"], s["classes"], s["hidden"], s["layers"], 0.0, s["relations"], num_bases), 33)
    model = RGCN(s["f"], s["classes"], s["hidden"], s["layers"], 0.0, s["relations"], num_bases)
    model.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return x, y, ei, et, model, ref


# ---- the restatement, pinned ------------------------------------------------------------------------------------------

def planted_rows():
    """rows[r, j, 0] = (r + 1) * v_j with v = 1 .. 6: one channel, so every number below is scalar arithmetic."""
    v = torch.arange(1, 7, dtype=torch.float64)
    return torch.stack([(r + 1) * v for r in range(PLANTED_R)])[:, :, None]


def test_restatement_reproduces_hand_computed_numbers():
    """target 0: (1 * 2 + 1 * 3 + 1 * 4) / 3 = 3 (one relation: the plain mean). target 1: 1 * 1 + 2 * 3 + 3 * 4 = 19 (three
    relations, one edge each: every weight is 1). target 2: relation 1 twice from node 4, (2 * 5 + 2 * 5) / 2 = 10, plus
    relation 0 once, 1 * 5: 15. target 3: its self-loop of relation 2, 3 * 4 = 12. Nodes 4 and 5: no in-edge, 0. With
    aggr="add" target 0 gets 9 and target 2 gets 25; the others had one edge per relation and stay."""
    ei, n = graph_of("planted")
    et = edge_type_of("planted", PLANTED_R)
    rows = planted_rows()
    assert aggregate(rows, n, ei[0], ei[1], et).flatten().tolist() == [3.0, 19.0, 15.0, 12.0, 0.0, 0.0]
    assert aggregate(rows, n, ei[0], ei[1], et, "add").flatten().tolist() == [9.0, 19.0, 25.0, 12.0, 0.0, 0.0]
    assert aggregate(rows, n, ei[0], ei[1], et, "sum").flatten().tolist() == [9.0, 19.0, 25.0, 12.0, 0.0, 0.0]
    assert int((et == PLANTED_R - 1).sum()) == 0                          # the relation that owns no edge
    _, cnt = slot_counts("planted", PLANTED_R)
    assert cnt.tolist() == [3, 3, 3, 1, 1, 1, 2, 2, 1, 1]                 # in slot order (= edge order here)


def test_restatement_layer_follows_the_formula():
    """RefRGCNConv against the definition spelled out edge by edge in Python floats, with and without a basis."""
    ei, n = graph_of("planted")
    et = edge_type_of("planted", PLANTED_R)
    x = f32_exact((n, 3), torch.Generator().manual_seed(1))
    for B in (None, 2):
        ref = randomize(RefRGCNConv(3, 2, PLANTED_R, num_bases=B), 2)
        W = ref.weight if B is None else torch.stack([sum(ref.comp[r, b] * ref.weight[b] for b in range(B))
                                                      for r in range(PLANTED_R)])
        want = x @ ref.root + ref.bias
        for i in range(n):
            for r in range(PLANTED_R):
                into = [e for e in range(ei.size(1)) if int(ei[1, e]) == i and int(et[e]) == r]
                if into:
                    want[i] = want[i] + sum(x[int(ei[0, e])] @ W[r] for e in into) / len(into)
        assert torch.allclose(ref(x, ei, et), want, rtol=0, atol=1e-12)


def test_restatement_sums_in_either_order():
    for graph in ("random", "planted"):
        R = PLANTED_R if graph == "planted" else 3
        case = mix_case(2, 4, R, graph)
        a, b = run_mix(case, R, graph, "mean"), run_mix(case, R, graph, "mean", reverse=True)
        assert max(shares_of(b, a, MIX_NAMES).values()) < 1e-6


def test_one_relation_is_the_plain_mean():
    """R = 1: the mean per (target, relation) is SAGE's mean over the in-edges."""
    ei, n = graph_of("random")
    h = f32_exact((n, 5), torch.Generator().manual_seed(3))
    got = aggregate(select_rows(h, 1), n, ei[0], ei[1], edge_type_of("random", 1))
    deg = torch.bincount(ei[1], minlength=n).clamp(min=1).double()
    want = torch.zeros(n, 5, dtype=torch.float64).index_add(0, ei[1], h[ei[0]]) / deg[:, None]
    assert torch.allclose(got, want, rtol=0, atol=1e-12)


# ---- registry and module layout ----------------------------------------------------------------------------------------

def test_registry():
    from rgb_experiment_amd import nn as product_nn
    from rgb_experiment_amd.dist import experiment as dist_experiment
    from rgb_experiment_amd.initial_params import InitialParameters
    from rgb_experiment_amd.models import MODELS, REGISTRY
    assert MODELS["rgcn"] is RGCN and "rgcn" not in REGISTRY
    assert "rgcn" not in dist_experiment.SUPPORTED
    assert "rgcn" not in [str(m).lower() for m in InitialParameters().model_names]
    assert "RGCNConv" in product_nn.__all__ and product_nn.RGCNConv is RGCNConv
    assert list(inspect.signature(RGCN.__init__).parameters)[1:] == [
        "input_dim", "output_dim", "hidden_unit", "num_layers", "dropout_rate", "num_relations", "num_bases"]
    assert list(inspect.signature(RGCN.forward).parameters)[1:] == ["x", "edge_index", "edge_type"]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("root_weight", [True, False])
@pytest.mark.parametrize("num_bases", [None, 2])
def test_parameter_names_shapes_and_strict_loading(num_bases, root_weight, bias):
    conv = RGCNConv(6, 7, 3, num_bases=num_bases, root_weight=root_weight, bias=bias)
    want = {"weight": (num_bases or 3, 6, 7)}
    if num_bases:
        want["comp"] = (3, num_bases)
    if root_weight:
        want["root"] = (6, 7)
    if bias:
        want["bias"] = (7,)
    assert {k: tuple(v.shape) for k, v in conv.named_parameters()} == want
    assert sorted(conv.state_dict()) == sorted(want)
    if bias:
        assert conv.bias.abs().max().item() == 0.0
    assert conv.weight.abs().max().item() > 0.0
    ref = randomize(RefRGCNConv(6, 7, 3, num_bases=num_bases, root_weight=root_weight, bias=bias), 4)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    back = RefRGCNConv(6, 7, 3, num_bases=num_bases, root_weight=root_weight, bias=bias)
    back.load_state_dict({k: v.double() for k, v in conv.state_dict().items()}, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), ref.state_dict().values()))


@pytest.mark.parametrize("num_bases", [None, 3])
def test_model_layout(num_bases):
    x, y, ei, et, model, ref = model_case(num_bases)
    s = MODEL_SHAPE
    assert len(model.convs) == s["layers"] and all(isinstance(c, RGCNConv) for c in model.convs)
    assert [(c.in_channels, c.out_channels) for c in model.convs] == [(16, 12), (12, 12), (12, 5)]
    assert sorted(model.state_dict()) == sorted(ref.state_dict())
    back = copy.deepcopy(ref)
    back.load_state_dict({k: v.double() for k, v in model.state_dict().items()}, strict=True)
    res = ref(x, ei, et)
    assert set(res) == {"out", "emb"} and res["out"].shape == (s["n"], s["classes"])
    with pytest.raises(ValueError, match="num_layers"):
        RGCN(4, 3, 8, 0, 0.5, 2)


def test_mix_channels_pads_what_the_layout_does_not_take():
    assert RGCNConv(4, 67, 3, num_bases=2).mix_channels() == 68
    assert RGCNConv(4, 130, 3, num_bases=2).mix_channels() == 132
    assert RGCNConv(4, 64, 3, num_bases=2).mix_channels() == 64
    assert RGCNConv(4, 7, 3, num_bases=65).mix_channels() is None        # beyond the head count: the select form
    assert RGCNConv(4, 300, 3, num_bases=2).mix_channels() is None
    assert RGCNConv(4, 7, 3).mix_channels() is None


# ---- refusals ------------------------------------------------------------------------------------------------------

class HostCSR:
    def __init__(self, nnz, N):
        self.nnz, self.N = nnz, N


class HostGraph:
    def __init__(self, n, e, loops_mode=0):
        self.N, self.E, self.loops_mode = n, e, loops_mode
        self.fwd = HostCSR(e, n)


def test_layer_refusals():
    with pytest.raises(NotImplementedError, match="num_blocks"):
        RGCNConv(4, 3, 2, num_blocks=2)
    with pytest.raises(ValueError, match="in_channels"):
        RGCNConv((4, 4), 3, 2)
    with pytest.raises(ValueError, match="in_channels"):
        RGCNConv(None, 3, 2)
    for aggr in ("max", "min", "mul", None):
        with pytest.raises(ValueError, match="aggr"):
            RGCNConv(4, 3, 2, aggr=aggr)
    for aggr in ("mean", "add", "sum"):
        RGCNConv(4, 3, 2, aggr=aggr)
    with pytest.raises(ValueError):
        RGCNConv(4, 3, 0)
    conv = RGCNConv(4, 3, 2)
    x, ei, et = torch.randn(5, 4), torch.tensor([[0, 1, 2], [1, 2, 3]]), torch.tensor([0, 1, 0])
    with pytest.raises(ValueError, match="featureless"):
        conv(None, ei, et)
    with pytest.raises(ValueError, match="edge_type"):
        conv(x, ei, None)
    with pytest.raises(ValueError, match="edge_type"):
        conv(x, ei, et[:2])
    with pytest.raises(ValueError, match="edge_type"):
        conv(x, ei, et.to(torch.int32))
    with pytest.raises(ValueError, match="in_channels"):
        conv(torch.randn(5, 3), ei, et)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(x, ei, et)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RGCNConv(4, 3, 2, num_bases=2)(x, ei, et)


def test_operator_refusals():
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, LOOPS_REMOVE_ADD

    class Partitioned:
        is_distributed = True
    et = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no node-partitioned form"):
        ops.rgcn_aggregate(torch.zeros(4, 8), Partitioned(), et, 2)
    with pytest.raises(RuntimeError, match="no node-partitioned form"):
        ops.typed_view(Partitioned(), et, 2)
    graph = HostGraph(4, 10)
    with pytest.raises(ValueError, match="aggr"):
        ops.rgcn_aggregate(torch.zeros(4, 8), graph, et, 2, aggr="max")
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.rgcn_aggregate(torch.zeros(4, 7), graph, et, 2)               # 7 columns are no 2 blocks
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.rgcn_aggregate(torch.zeros(3, 8), graph, et, 2)
    with pytest.raises(RuntimeError, match="comp"):
        ops.rgcn_aggregate(torch.zeros(4, 8), graph, et, 2, comp=torch.zeros(3, 2))
    with pytest.raises(RuntimeError, match="y0"):
        ops.rgcn_aggregate(torch.zeros(4, 8), graph, et, 2, y0=torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rgcn_aggregate(torch.zeros(4, 8), graph, et, 2)
    for mode in (LOOPS_ADD_REMAINING, LOOPS_REMOVE_ADD):
        with pytest.raises(RuntimeError, match="LOOPS_KEEP"):
            ops.typed_view(HostGraph(4, 10, loops_mode=mode), et, 2)
    with pytest.raises(ValueError, match="num_relations"):
        ops.typed_view(graph, et, 0)
    for bad in (et[:9], et.to(torch.int32), et.view(2, 5), None):
        with pytest.raises(ValueError, match="edge_type"):
            ops.typed_view(graph, bad, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.typed_view(graph, et, 2)


def test_select_form_refuses_an_index_range_beyond_int32():
    """N * R >= 2^31 is refused before anything is launched or even moved: operands without storage suffice."""
    from rgb_experiment_amd import ops
    N, R = 2 ** 28, 8
    h = torch.empty((N, R * 1), dtype=torch.float32, device="meta")
    with pytest.raises(RuntimeError, match="beyond int32"):
        ops.rgcn_aggregate(h, HostGraph(N, 10), torch.zeros(10, dtype=torch.int64), R)
    small = torch.empty((N, 7), dtype=torch.float32, device="meta")      # R = 7: N * R < 2^31, the device check is next
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rgcn_aggregate(small, HostGraph(N, 10), torch.zeros(10, dtype=torch.int64), 7)


# ---- experiment(use_edge_type=...) ---------------------------------------------------------------------------------------

class TypedModel(nn.Module):
    """A caller's module whose forward takes edge_type (dense work only: it runs on the CPU)."""

    def __init__(self, f, r, c):
        super().__init__()
        self.lin, self.rel = nn.Linear(f, c), nn.Embedding(r, c)
        self.seen = None

    def forward(self, x, edge_index, edge_type):
        self.seen = edge_type
        h = self.lin(x) + self.rel(edge_type).mean(0)
        return {"out": F.log_softmax(h, dim=1), "emb": h}


def _data(with_type, types=None):
    from rgb_experiment_amd.data import Data
    g = torch.Generator().manual_seed(5)
    n = 60
    extra = {}
    if with_type:
        extra["edge_type"] = torch.randint(0, 3, (300,), generator=torch.Generator().manual_seed(6)) if types is None \
            else types
    return Data(x=torch.randn(n, 8, generator=g), y=torch.randint(0, 3, (n,), generator=g),
                edge_index=torch.randint(0, n, (2, 300), generator=g), **extra)


RGCN_INIT = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0, "num_relations": 3}


def test_experiment_refusals():
    sig = inspect.signature(__import__("rgb_experiment_amd").experiment).parameters
    assert sig["use_edge_type"].default is False
    assert sig["use_edge_attr"].default is False and sig["use_edge_weight"].default is False
    run, rgcn = G._run, dict(model_name="rgcn", init=RGCN_INIT, use_edge_type=True)
    for name in ("mlp", "gcn", "graphsage", "gat", "gin", "gine", "dagnn", "resgated", "transformer"):
        with pytest.raises(ValueError, match="takes no edge types"):
            run(_data(True), model_name=name, use_edge_type=True)
    with pytest.raises(ValueError, match="takes no edge_type"):
        run(_data(True), model=G.PlainModel(8, 3), use_edge_type=True)
    with pytest.raises(ValueError, match="to_undirected"):
        run(_data(True), to_undirected_graph=True, **rgcn)
    with pytest.raises(NotImplementedError, match="partitioned"):
        run(_data(True), distributed=True, **rgcn)
    with pytest.raises(NotImplementedError):  # the name checks stay in front
        run(_data(True), model_name="fagcn", use_edge_type=True)
    with pytest.raises(ValueError, match="unknown model_name"):
        run(_data(True), model_name="nonesuch", use_edge_type=True)
    with pytest.raises(NotImplementedError):
        run(_data(True), print_pics=True, **rgcn)
    # data.edge_type must be int64 [E]
    with pytest.raises(ValueError, match="needs data.edge_type"):
        run(_data(False), **rgcn)
    with pytest.raises(ValueError, match="needs data.edge_type"):
        run(_data(True, torch.zeros(300)), **rgcn)
    with pytest.raises(ValueError, match="needs data.edge_type"):
        run(_data(True, torch.zeros(300, dtype=torch.int32)), **rgcn)
    with pytest.raises(ValueError, match=r"\[E\]"):
        run(_data(True, torch.zeros(299, dtype=torch.int64)), **rgcn)
    with pytest.raises(ValueError, match=r"\[E\]"):
        run(_data(True, torch.zeros(300, 1, dtype=torch.int64)), **rgcn)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # well-formed: the device check is next
        run(_data(True), **rgcn)
    # the other two edge flags keep their refusals
    with pytest.raises(ValueError, match="takes no edge attributes"):
        run(_data(True), model_name="rgcn", init=RGCN_INIT, use_edge_attr=True)
    with pytest.raises(ValueError, match="takes no edge weights"):
        run(_data(True), model_name="rgcn", init=RGCN_INIT, use_edge_weight=True)


def test_a_callers_model_receives_edge_type():
    data = _data(True)
    model = TypedModel(8, 3, 3)
    before = copy.deepcopy(model.rel.weight.detach())
    res = G._run(data, model=model, use_edge_type=True)
    assert model.seen is not None and model.seen.dtype == torch.int64 and torch.equal(model.seen, data.edge_type)
    assert len(res["history"]["train_loss"]) == 4 and not torch.equal(model.rel.weight.detach(), before)
    with pytest.raises(TypeError):                                       # flag off: the argument is not passed
        G._run(data, model=TypedModel(8, 3, 3))


def test_an_unused_edge_type_attribute_changes_nothing():
    a, b = G._run(_data(False)), G._run(_data(True))
    assert a["history"] == b["history"] and a["ACC"] == b["ACC"]
    plain = lambda: (torch.manual_seed(3), G.PlainModel(8, 3))[1]
    c, d = G._run(_data(False), model=plain()), G._run(_data(True), model=plain())
    assert c["history"] == d["history"]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

NEW_ENTRIES = ("rgbx_rgcn_slot_norm_f32", "rgbx_rgcn_mix_supported", "rgbx_rgcn_mix_fwd_f32", "rgbx_rgcn_mix_bwd_src_f32",
               "rgbx_rgcn_mix_bwd_coef_f32")


def loaded_lib():
    from rgb_experiment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_abi_declares_and_exports_the_new_entries():
    from rgb_experiment_amd import _lib
    raw = open(os.path.join(ROOT, "include", "rgbx_hip.h")).read()
    assert "RGCNConv.forward [PyG]" in raw and "masked_edge_index" in raw   # the PyG lines the family replaces
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(rgbx_[a-z0-9_]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS, name
        params = re.search(name + r"\s*\(([^)]*)\)", text).group(1)       # one ctypes argument per declared parameter
        assert len(_lib.SIGNATURES[name]) == len([a for a in params.split(",") if a.strip()]), name
    assert loaded_lib().rgbx_version() == 501


def test_mix_supported_over_the_gpu_grid():
    lib = loaded_lib()
    for B, C in MIX_PAIRS + SWEEP_PAIRS:
        assert lib.rgbx_rgcn_mix_supported(B, C), (B, C)
    for C in range(1, 301):                                               # the widths of the shared lane layout
        assert bool(lib.rgbx_rgcn_mix_supported(2, C)) == bool(lib.rgbx_transformer_supported(2, C)), C
    assert not lib.rgbx_rgcn_mix_supported(2, PADDED_WIDTH) and lib.rgbx_rgcn_mix_supported(2, PADDED_WIDTH + 1)
    assert lib.rgbx_rgcn_mix_supported(64, 8) and not lib.rgbx_rgcn_mix_supported(65, 8)
    assert not lib.rgbx_rgcn_mix_supported(0, 8) and not lib.rgbx_rgcn_mix_supported(-1, 8)
    assert not lib.rgbx_rgcn_mix_supported(2, 0)
    # vector widths as attn_common.h's pick_vec chooses them on aligned rows: all three occur in the grid
    assert {4 if C % 4 == 0 else (2 if C % 2 == 0 else 1) for C in WIDTHS} == {1, 2, 4}
    assert {4 if C % 4 == 0 else (2 if C % 2 == 0 else 1) for _, C in SWEEP_PAIRS} == {1, 2, 4}
    pow2ceil = lambda v: 1 << (v - 1).bit_length()
    chunks = lambda B, C: -(-B // min(B, 64 // pow2ceil(-(-C // (4 if C % 4 == 0 else (2 if C % 2 == 0 else 1))))))
    assert chunks(30, 16) > 1 and chunks(8, 64) > 1 and chunks(2, 7) == 1  # head counts in several chunks, and in one


def test_new_entries_validate_their_arguments():
    lib = loaded_lib()
    p = 0x10000  # 16-byte aligned, non-null, never dereferenced: every call below returns before a launch

    def norm(**kw):
        a = dict(rowptr=p, etype=p, w=p, N=10, R=3)
        a.update(kw)
        return lib.rgbx_rgcn_slot_norm_f32(a["rowptr"], a["etype"], a["w"], a["N"], a["R"], None, None)
    assert norm(rowptr=None) == -1 and b"null" in lib.rgbx_last_error_string()
    assert norm(etype=None) == -1 and norm(w=None) == -1
    assert norm(R=0) == -1 and b"num_relations" in lib.rgbx_last_error_string()
    assert norm(R=-2) == -1 and norm(N=-1) == -1
    assert norm(N=2 ** 31) == -2
    assert norm(w=p + 2) == -3 and norm(etype=p + 1) == -3
    assert norm(N=0) == 0 and norm(N=0, rowptr=None) == 0

    def fwd(**kw):
        a = dict(rowptr=p, col=p, etype=p, w=p, comp=p, h=p, ldh=128, y0=p, ldy=64, out=p + 0x100000, ldo=64, N=10, R=3,
                 B=2, C=64)
        a.update(kw)
        return lib.rgbx_rgcn_mix_fwd_f32(a["rowptr"], a["col"], a["etype"], a["w"], a["comp"], a["h"], a["ldh"], a["y0"],
                                         a["ldy"], a["out"], a["ldo"], a["N"], a["R"], a["B"], a["C"], None, None)
    for name in ("rowptr", "col", "etype", "w", "comp", "h", "out"):
        assert fwd(**{name: None}) == -1 and b"null" in lib.rgbx_last_error_string(), name
    assert fwd(ldh=127) == -1 and b"leading dimension" in lib.rgbx_last_error_string()
    assert fwd(ldo=63) == -1 and fwd(ldy=8) == -1
    assert fwd(out=p) == -1 and b"alias" in lib.rgbx_last_error_string()
    assert fwd(R=0) == -1 and b"num_relations" in lib.rgbx_last_error_string()
    assert fwd(N=-1) == -1 and fwd(B=0) == -1 and fwd(C=0) == -1
    assert fwd(N=2 ** 31) == -2 and fwd(R=2 ** 30, B=2) == -2             # RGBX_E_RANGE
    assert fwd(C=67, ldh=134, ldy=67, ldo=67) == -5 and fwd(B=65, ldh=65 * 64) == -5   # RGBX_E_SHAPE
    assert fwd(h=p + 2) == -3 and b"aligned" in lib.rgbx_last_error_string()
    assert fwd(comp=p + 1) == -3 and fwd(w=p + 3) == -3 and fwd(etype=p + 2) == -3 and fwd(y0=p + 2) == -3
    # C = 256 needs 4 floats per lane: 16-byte pointers and leading dimensions that are multiples of 4
    wide = dict(C=256, ldh=512, ldy=256, ldo=256)
    assert fwd(**{**wide, "h": p + 8}) == -5 and b"lanes" in lib.rgbx_last_error_string()
    assert fwd(**{**wide, "ldh": 514}) == -5
    assert fwd(N=0) == 0 and fwd(N=0, rowptr=None) == 0

    def src(**kw):
        a = dict(etype_t=p, w_t=p, comp=p, gout=p, ldg=64, g_h=p + 0x100000, ldgh=128, N=1000, R=3, B=2, C=64)
        a.update(kw)
        return lib.rgbx_rgcn_mix_bwd_src_f32(p, p, a["etype_t"], a["w_t"], a["comp"], a["gout"], a["ldg"], a["g_h"],
                                             a["ldgh"], a["N"], a["R"], a["B"], a["C"], None, None)
    for name in ("etype_t", "w_t", "comp", "gout", "g_h"):
        assert src(**{name: None}) == -1, name
    assert src(ldg=63) == -1 and src(ldgh=127) == -1 and src(g_h=p) == -1
    assert src(R=0) == -1 and src(B=-1) == -1
    assert src(gout=p + 2) == -3 and src(g_h=p + 0x100001) == -3 and src(comp=p + 2) == -3
    assert src(C=130, ldg=130, ldgh=260) == -5
    assert src(N=2 ** 31) == -2 and src(N=0) == 0

    def coef(**kw):
        a = dict(w=p, h=p, ldh=128, gout=p, ldg=64, d=p, N=1000, R=3, B=2, C=64)
        a.update(kw)
        return lib.rgbx_rgcn_mix_bwd_coef_f32(p, p, a["w"], a["h"], a["ldh"], a["gout"], a["ldg"], a["d"], a["N"], a["R"],
                                              a["B"], a["C"], None, None)
    for name in ("w", "h", "gout", "d"):
        assert coef(**{name: None}) == -1, name
    assert coef(ldh=100) == -1 and coef(ldg=32) == -1
    assert coef(R=0) == -1 and coef(d=p + 2) == -3 and coef(h=p + 1) == -3
    assert coef(C=67) == -5 and coef(B=100, ldh=6400) == -5
    assert coef(N=2 ** 31) == -2 and coef(N=0) == 0


# ---- preconditions of the GPU cases ----------------------------------------------------------------------------------

def test_graphs_and_types_have_what_the_cases_need():
    from rgb_experiment_amd.graph import LONG_ROW_SLOTS as product_threshold
    assert LONG_ROW_SLOTS == product_threshold
    for R in RELATIONS:
        for name in ("degrees", "powerlaw", "random"):
            et = edge_type_of(name, R)
            assert et.dtype == torch.int64 and int(et.min()) == 0 and int(et.max()) == max(R - 2, 0)
            used = torch.bincount(et, minlength=R)
            assert bool((used[:max(R - 1, 1)] > 0).all()) and (R == 1 or int(used[R - 1]) == 0)
    ei, n = graph_of("degrees")
    _, cnt = slot_counts("degrees", 3)
    rowptr = slots_of("degrees")[2]
    hub = cnt[rowptr[5]:rowptr[6]]                                        # the row of T + 1 slots: counts beyond one chunk's
    assert hub.numel() == LONG_ROW_SLOTS + 1 and int(hub.max()) > 64 and int(hub.sum() > 0)
    for R in RELATIONS:                                                   # every slot counts itself; a row's weights sum to
        for name in ("degrees", "powerlaw", "random", "planted") if R == 3 else ("degrees",):   # its number of relations
            RR = PLANTED_R if name == "planted" else R
            et, c = slot_counts(name, RR)
            assert int(c.min()) >= 1
            dst = graph_of(name)[0][1][slots_of(name)[3]]
            per_row = torch.zeros(graph_of(name)[1], dtype=torch.float64).index_add(0, dst, 1.0 / c.double())
            kinds = torch.unique(dst * RR + et).numel()
            assert abs(per_row.sum().item() - kinds) < 1e-9
    # a relation holds about E / R slots: always a hub row of the grouping by relation on the two large graphs
    assert int(torch.bincount(edge_type_of("powerlaw", 7)).min()) > LONG_ROW_SLOTS


@pytest.mark.parametrize("B,C,R,graph,aggr", MIX_CASES)
def test_mix_case_is_well_posed(B, C, R, graph, aggr):
    aggr = "add" if aggr == "sum" else aggr
    want = mix_reference(B, C, R, graph, aggr)
    got = run_mix(mix_case(B, C, R, graph), R, graph, aggr, dtype=torch.float32, reverse=True)
    shares = shares_of(got, want, MIX_NAMES)
    assert max(shares.values()) < WELL_POSED_SHARE, shares
    if R > 1 and graph != "planted":
        assert want[1][1][R - 1].abs().max().item() == 0.0                # the relation without an edge
    if graph == "no_edges":
        assert torch.equal(want[0], mix_case(B, C, R, graph)[2])          # out == y0


@pytest.mark.parametrize("C,R,graph,aggr", SELECT_CASES)
def test_select_case_is_well_posed(C, R, graph, aggr):
    want = select_reference(C, R, graph, aggr)
    got = run_select(select_case(C, R, graph), R, graph, aggr, dtype=torch.float32, reverse=True)
    shares = shares_of(got, want, SELECT_NAMES)
    assert max(shares.values()) < WELL_POSED_SHARE, shares


def module_shares(ref, forward, cot_seed):
    """A reference module in float64 against its float32 copy run with reversed sums: shares of the tolerances of the
    output and of every parameter gradient."""
    low = copy.deepcopy(ref).float()
    want, got = forward(ref, torch.float64, False), forward(low, torch.float32, True)
    cot = f32_exact(tuple(want.shape), torch.Generator().manual_seed(cot_seed))
    (want * cot).sum().backward()
    (got * cot.float()).sum().backward()
    shares = {"forward": share_of_tolerance(got, want, FWD_TOL)}
    for (name, p), q in zip(ref.named_parameters(), low.parameters()):
        shares[name] = share_of_tolerance(q.grad, p.grad, GRAD_TOL)
    return shares


@pytest.mark.parametrize("name", sorted(LAYER_CASES))
def test_layer_case_is_well_posed(name):
    x, ei, et, ref = layer_case(name)
    shares = module_shares(ref, lambda m, dt, rev: m(x.to(dt), ei, et, rev), 17)
    assert max(shares.values()) < WELL_POSED_SHARE, shares


@pytest.mark.parametrize("num_bases", [None, 3])
def test_model_case_is_well_posed(num_bases):
    x, y, ei, et, model, ref = model_case(num_bases)
    ref.train()
    shares = module_shares(ref, lambda m, dt, rev: m(x.to(dt), ei, et, rev)["out"], 18)
    assert max(shares.values()) < WELL_POSED_SHARE, shares
