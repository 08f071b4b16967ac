"""GINEConv on the host: a float64 restatement of the layer (message relu(x_j + e_ji) summed over the in-edges AS GIVEN,
root term (1 + eps) x_i, then nn) pinned by numbers derived by hand; registry, module layout (PyG's names, strict
state_dict loading), the slot permutation of the edge attributes, refusals, the use_edge_attr keyword of experiment()
and the C ABI of the new entry points; and the case builders tests/test_gpu_gine.py feeds to the HIP kernels, with the
checks that keep those cases well-posed. No GPU needed.

Well-posedness. relu has a kink: a relu input that is positive in float64 and non-positive in float32 (or the other way
round) changes a whole gradient entry, which no tolerance covers. The operator cases avoid this by construction: x and e
are exactly representable in float32, the float32 add x_j + e_p is correctly rounded, so it has the sign of the exact
sum (asserted for every slot and channel), and the only zeros are the planted ties x_j = -e_p (asserted too). The mask is
then the same in float32 and float64 and what is left is summation error: every case is run through the restatement in
float32 on the CPU with the edges in REVERSED order and has to stay within a QUARTER of the GPU test's tolerances
(forward 1e-4, gradients 2e-4, times max(1, |ref|max)) of the float64 result.

In the layer and model cases e = lin(edge_attr) is a float32 product of D terms and, in the model, x is the output of
float32 layers (a product, BatchNorm), so a relu input close to zero CAN flip. Each such case asserts that no relu input
of the float64 run lies within a margin of zero; the margin is derived below (relu_margin) from the standard error bound
of a float32 dot product and of BatchNorm's affine map. Seeds are fixed so that the reference alone satisfies this; a
case that does not fails, it is never skipped."""
import copy
import functools
import inspect
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from rgb_experiment_amd.models import GINE             # without the feature this file fails here, at import
from rgb_experiment_amd.nn import GINEConv

import test_transformer_host as T
from test_transformer_host import FWD_TOL, GRAD_TOL, LONG_ROW_SLOTS, WELL_POSED_SHARE, f32_exact, share_of_tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------

def aggregate(x, e, n, src, dst, eps=None):
    """out [n, C] = (1 + eps) x + sum over the edges (src -> dst) as given of relu(x[src] + e), e [E, C] one row per
    edge in the order of the edge list, in the precision of the inputs. eps=None: no root term. A node without in-edges
    gets the root term alone. The sum runs in the order of the edge list; torch's relu has gradient 0 at 0."""
    msg = torch.relu(x.index_select(0, src) + e)
    out = torch.zeros(n, x.size(1), dtype=x.dtype).index_add(0, dst, msg)
    return out if eps is None else out + (1 + eps) * x


def ref_block(fan_in, width):
    """models/gin.py's _block in float64 (Linear-ReLU-Linear-ReLU-BatchNorm)."""
    return nn.Sequential(nn.Linear(fan_in, width), nn.ReLU(), nn.Linear(width, width), nn.ReLU(),
                         nn.BatchNorm1d(width)).double()


class RefGINEConv(nn.Module):
    """float64 restatement of GINEConv, written from the formulas of the layer's contract; PyG's parameter names (nn.*,
    eps — a Parameter with train_eps, a buffer otherwise —, lin.* only with edge_dim). `relu_inputs` keeps x_j + e_ji
    of the last forward (what the well-posedness margin is asserted on)."""

    def __init__(self, nn_module, eps=0.0, train_eps=False, edge_dim=None, in_channels=None):
        super().__init__()
        self.nn = nn_module
        if train_eps:
            self.eps = nn.Parameter(torch.tensor([float(eps)], dtype=torch.float64))
        else:
            self.register_buffer("eps", torch.tensor([float(eps)], dtype=torch.float64))
        self.lin = nn.Linear(edge_dim, in_channels).double() if edge_dim is not None else None
        self.relu_inputs = None

    def forward(self, x, ei, ea, reverse=False):
        src, dst = ei[0], ei[1]
        e = ea if self.lin is None else self.lin(ea)
        self.relu_inputs = (x.index_select(0, src) + e).detach()
        if reverse:
            src, dst, e = src.flip(0), dst.flip(0), e.flip(0)
        return self.nn(aggregate(x, e, x.size(0), src, dst, self.eps))


class RefGINE(nn.Module):
    """models/gine.py in float64: encoder, num_layers x GINEConv(block, train_eps=True, edge_dim), lin1 -> ReLU ->
    dropout -> lin2; the product's module names."""

    def __init__(self, input_dim, output_dim, hidden_unit, num_layers, dropout_rate, edge_dim):
        super().__init__()
        self.dropout_rate = dropout_rate
        self.encoder = nn.Linear(input_dim, hidden_unit).double()
        self.convs = nn.ModuleList(RefGINEConv(ref_block(hidden_unit, hidden_unit), train_eps=True, edge_dim=edge_dim,
                                               in_channels=hidden_unit) for _ in range(num_layers))
        self.lin1 = nn.Linear(hidden_unit, hidden_unit).double()
        self.lin2 = nn.Linear(hidden_unit, output_dim).double()
        self.conv_inputs = []

    def forward(self, x, ei, ea, reverse=False):
        x = self.encoder(x)
        self.conv_inputs = []
        for conv in self.convs:
            self.conv_inputs.append(x.detach())
            x = conv(x, ei, ea, reverse)
        x = F.dropout(F.relu(self.lin1(x)), p=self.dropout_rate, training=self.training)
        x = self.lin2(x)
        return {"out": F.log_softmax(x, dim=1), "emb": x}


# ---- graphs ---------------------------------------------------------------------------------------------------------

DEGREES = (0, 1, 64, 65, LONG_ROW_SLOTS, LONG_ROW_SLOTS + 1)   # T = LONG_ROW_SLOTS: the last row a wave sums alone, T + 1 is split
SMALL_GRAPHS = ("n1", "n2", "n3")
GRAPH_NAMES = T.GRAPH_NAMES                                     # no_edges, powerlaw, random


@functools.lru_cache(maxsize=None)
def graph_of(name):
    """(edge_index, n). no_edges / powerlaw / random: tests/test_transformer_host.graph_of. `degrees`: node k < 6 has
    exactly DEGREES[k] in-edges and node 6 + k exactly DEGREES[k] out-edges (the other endpoints are the nodes from 12
    on, one edge each), in a shuffled edge list. n1 / n2 / n3: graphs of one, two and three nodes with self-loops and
    duplicates."""
    if name in GRAPH_NAMES:
        return T.graph_of(name)
    if name == "degrees":
        src, dst = [], []
        for k, d in enumerate(DEGREES):
            others = torch.arange(12, 12 + d)
            src += [others, torch.full((d,), 6 + k)]
            dst += [torch.full((d,), k), others]
        ei = torch.stack([torch.cat(src), torch.cat(dst)])
        return ei[:, torch.randperm(ei.size(1), generator=torch.Generator().manual_seed(5))].contiguous(), 12 + max(DEGREES)
    if name == "n1":
        return torch.tensor([[0, 0], [0, 0]]), 1
    if name == "n2":
        return torch.tensor([[0, 1, 0, 0], [1, 0, 0, 1]]), 2
    if name == "n3":
        return torch.tensor([[0, 1, 2, 2, 1], [1, 2, 0, 0, 1]]), 3
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def slots_of(name):
    """(src, dst, rowptr, order): slot p of the target-grouped CSR is edge order[p] (a stable grouping by target, which
    the device's CSR build is: tests/test_gpu_parity.py::test_csr_build_bit_exact)."""
    ei, n = graph_of(name)
    order = torch.argsort(ei[1], stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(ei[1], minlength=n), 0)
    return ei[0], ei[1], rowptr, order


# ---- operator cases shared with tests/test_gpu_gine.py ----------------------------------------------------------------

WIDTHS = [1, 4, 5, 7, 40, 64, 66, 128, 132, 256]   # every vector width (1, 2, 4) and 64, 8, 4, 2, 1 rows per wave-instruction
DEGREE_WIDTHS = [5, 66, 132]                        # one width per vector width on the `degrees` graph
SMALL_WIDTHS = [3, 64]
BLOCKED_WIDTH = 300                                 # above 256: column blocks of 256 and 44
EPS = 0.25                                          # 1 + eps is exact in float32
TIE_EVERY = 7                                       # every 7th edge carries one planted tie x_j[c] = -e_p[c]
NAMES = ("forward", "g_x", "g_e", "g_eps")


def tie_positions(n_edges, C):
    k = torch.arange(0, n_edges, TIE_EVERY)
    return k, (k // TIE_EVERY) % C


@functools.lru_cache(maxsize=6)
def operator_case(C, graph_name):
    """x [n, C], e [E, C] (one row per edge, in the order of the edge list), the cotangent [n, C]: float64, fp32-exact,
    N(0, 1); every TIE_EVERY-th edge has one channel with e = -x_j exactly (the negation of a float32 is one), and
    those planted ties are the only zeros of x_j + e."""
    ei, n = graph_of(graph_name)
    g = torch.Generator().manual_seed(6000 + C)
    x, cot = f32_exact((n, C), g), f32_exact((n, C), g)
    e = f32_exact((ei.size(1), C), g)
    xj = x[ei[0]]
    chance = (xj + e) == 0                     # two draws that happen to cancel: made 2 x_j (or 1), exact and non-zero
    e[chance] = torch.where(xj[chance] == 0, torch.ones_like(xj[chance]), xj[chance])
    k, c = tie_positions(ei.size(1), C)
    e[k, c] = -xj[k, c]
    return x, e, cot


def run_formula(case, graph_name, dtype=torch.float64, reverse=False):
    """The restatement's aggregation on a case in `dtype`: (out [n, C], [g_x, g_e, g_eps]), g_e in the order of the edge
    list. `reverse`: the edge list backwards, i.e. every row summed in the opposite order."""
    ei, n = graph_of(graph_name)
    src, dst = ei[0], ei[1]
    x, e = (t.to(dtype).clone().requires_grad_(True) for t in case[:2])
    eps = torch.tensor([EPS], dtype=dtype, requires_grad=True)
    if reverse:
        out = aggregate(x, e.flip(0), n, src.flip(0), dst.flip(0), eps)
    else:
        out = aggregate(x, e, n, src, dst, eps)
    (out * case[2].to(dtype)).sum().backward()
    return out.detach(), [x.grad, e.grad, eps.grad]


@functools.lru_cache(maxsize=6)
def reference(C, graph_name):
    """The float64 result of a case, computed once and shared (read-only) by the host and the GPU tests."""
    return run_formula(operator_case(C, graph_name), graph_name)


def shares_of(got, want):
    out = {"forward": share_of_tolerance(got[0], want[0], FWD_TOL)}
    for name, a, b in zip(NAMES[1:], got[1], want[1]):
        assert a.shape == b.shape
        out[name] = share_of_tolerance(a, b, GRAD_TOL) if b.numel() else 0.0   # g_e of a graph without edges is [0, C]
    return out


def check_masks_agree(case, graph_name):
    """The float32 add x_j + e_p has the sign of the exact sum in every slot and channel, and the planted ties are the
    only zeros: the relu mask is then the same in float32 and in float64. -> the number of ties."""
    ei, _ = graph_of(graph_name)
    x, e = case[:2]
    z64 = x[ei[0]] + e                                       # exact: both are float32 values, float64 holds their sum
    z32 = x.float()[ei[0]] + e.float()
    assert torch.equal(torch.sign(z32).double(), torch.sign(z64))
    k, c = tie_positions(ei.size(1), x.size(1))
    planted = torch.zeros_like(z64, dtype=torch.bool)
    planted[k, c] = True
    assert torch.equal(z64 == 0, planted)
    return int(planted.sum())


# ---- layer and model cases ----------------------------------------------------------------------------------------------

U32 = 2.0 ** -24                                    # unit roundoff of float32


def gamma(k):
    """k u / (1 - k u): the relative error bound of a float32 sum of k terms in any order (Higham, Accuracy and
    Stability of Numerical Algorithms, Lemma 3.1)."""
    return k * U32 / (1 - k * U32)


def relu_margin(conv, x, ei, ea, x_err=0.0):
    """An upper bound, per edge and channel, of |float32 relu input - float64 relu input| for a reference layer `conv`
    on float64 inputs. e = lin(ea) is a float32 dot product of D terms plus the bias: its error is at most
    gamma(D + 1) (|ea| |W|^T + |b|) for any order of summation and with or without fused multiply-adds; the add x_j + e
    rounds once more: u |x_j + e| <= u (|x_j| + |ea| |W|^T + |b|); with edge_dim=None e is exact, and a correctly rounded
    add of two exact operands has the sign of their sum: the margin is then x's own error alone.
    `x_err` (a number or a [n, C] tensor) bounds the error x itself arrives with (0 for an exact input)."""
    xj = x.index_select(0, ei[0]).abs()
    if conv.lin is None:  # both operands exact: a correctly rounded add keeps the sign, only x's own error counts
        return torch.zeros_like(xj) + (x_err if not torch.is_tensor(x_err) else x_err.index_select(0, ei[0]))
    D = ea.size(1)
    mag = ea.abs() @ conv.lin.weight.detach().abs().t() + conv.lin.bias.detach().abs()
    xe = x_err if not torch.is_tensor(x_err) else x_err.index_select(0, ei[0])
    return gamma(D + 1) * mag + U32 * (xj + mag) + xe


LAYER_N, LAYER_E, LAYER_F = 120, 500, 6
LAYER_WIDTHS = [7, 67, 130]                         # 67 and 130 are outside the kernels' widths: the layer pads them
LAYER_FLAGS = [(True, True), (True, False), (False, True), (False, False)]   # edge_dim set x train_eps


def layer_case(C, with_lin, train_eps):
    """(x float64 fp32-exact [n, C], edge_index, edge_attr [E, D or C], reference layer with nn = Linear(C, C) -> ReLU ->
    Linear(C, 5) and every parameter set to fp32-exact random values)."""
    from test_gpu_ggnn import rand_graph
    g = torch.Generator().manual_seed(8300 + C + 1000 * with_lin)
    ei = rand_graph(LAYER_N, LAYER_E, 8300, loops=5, dups=12)
    x = f32_exact((LAYER_N, C), g)
    ea = f32_exact((ei.size(1), LAYER_F if with_lin else C), g)
    net = nn.Sequential(nn.Linear(C, C), nn.ReLU(), nn.Linear(C, 5)).double()
    ref = RefGINEConv(net, eps=0.375, train_eps=train_eps, edge_dim=LAYER_F if with_lin else None, in_channels=C)
    with torch.no_grad():
        for key, prm in ref.named_parameters():
            if key != "eps":
                prm.copy_(f32_exact(prm.shape, g, prm.size(-1) ** -0.5 if key.endswith("weight") else 0.5))
    return x, ei, ea, ref


MODEL_SHAPE = dict(n=60, e=240, f=16, hidden=12, classes=5, layers=3, edge_dim=6)


def model_case():
    """(x, y, edge_index, edge_attr, the product's model on the CPU, the reference holding its parameters)."""
    from test_gpu_ggnn import rand_graph
    s = MODEL_SHAPE
    g = torch.Generator().manual_seed(9400)
    ei = rand_graph(s["n"], s["e"], 9400, loops=3, dups=6)
    x = f32_exact((s["n"], s["f"]), g)
    ea = f32_exact((ei.size(1), s["edge_dim"]), g)
    y = torch.randint(0, s["classes"], (s["n"],), generator=g)
    torch.manual_seed(9400)
    model = GINE(s["f"], s["classes"], s["hidden"], s["layers"], 0.0, s["edge_dim"])
    with torch.no_grad():  # biases and eps off zero, so that their paths are exercised
        for key, prm in model.named_parameters():
            if key.endswith("bias"):
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.3)
            if key.endswith("eps"):
                prm.copy_(torch.rand(prm.shape, generator=g) * 0.5)
    ref = RefGINE(s["f"], s["classes"], s["hidden"], s["layers"], 0.0, s["edge_dim"])
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()},
                        strict=True)
    return x, y, ei, ea, model, ref


# ---- the restatement is pinned -------------------------------------------------------------------------------------

def t64(rows):
    return torch.tensor(rows, dtype=torch.float64)


HAND_X = [[1, -2], [3, 0.5], [-1, 4], [7, -7]]


def test_restatement_on_a_path():
    """0 -> 1 -> 2, two channels, eps = 1/2, x = (1, -2), (3, 1/2), (-1, 4); e_01 = (1/2, 1), e_12 = (-4, 3/2). By hand:
      out_0 = 3/2 x_0                                                   = (3/2, -3)      (no in-edge: the root alone)
      out_1 = 3/2 (3, 1/2) + relu((1, -2) + (1/2, 1)) = (9/2, 3/4) + (3/2, 0)   = (6, 3/4)
      out_2 = 3/2 (-1, 4) + relu((3, 1/2) + (-4, 3/2)) = (-3/2, 6) + (0, 2)     = (-3/2, 8)
    With the cotangent all ones: g_e01 = (1, 0), g_e12 = (0, 1) (the masks); g_x0 = 3/2 + (1, 0), g_x1 = 3/2 + (0, 1),
    g_x2 = 3/2; g_eps = sum of all x = 1 - 2 + 3 + 1/2 - 1 + 4 = 11/2."""
    x = t64(HAND_X[:3]).requires_grad_(True)
    e = t64([[0.5, 1], [-4, 1.5]]).requires_grad_(True)
    eps = torch.tensor([0.5], dtype=torch.float64, requires_grad=True)
    out = aggregate(x, e, 3, torch.tensor([0, 1]), torch.tensor([1, 2]), eps)
    assert torch.equal(out, t64([[1.5, -3], [6, 0.75], [-1.5, 8]]))
    out.sum().backward()
    assert torch.equal(e.grad, t64([[1, 0], [0, 1]]))
    assert torch.equal(x.grad, t64([[2.5, 1.5], [1.5, 2.5], [1.5, 1.5]]))
    assert torch.equal(eps.grad, t64([5.5]))
    assert torch.equal(aggregate(x, e, 3, torch.tensor([0, 1]), torch.tensor([1, 2])).detach(),
                       t64([[0, 0], [1.5, 0], [0, 2]]))                 # eps=None: no root term


def test_restatement_duplicate_self_loop_isolated():
    """Edges 0 -> 1 twice (a duplicate, both with e = (1/2, 1)), 1 -> 1 (a self-loop, e = (-1, -1)), 1 -> 2
    (e = (-4, 3/2)); node 0 has no in-edge, node 3 no edge at all; eps = 1/2.
      out_1 = 3/2 (3, 1/2) + 2 relu((3/2, -1)) + relu((3, 1/2) + (-1, -1)) = (9/2, 3/4) + (3, 0) + (2, 0) = (19/2, 3/4)
      out_2 = (-3/2, 8) as on the path; out_0 = 3/2 x_0; out_3 = 3/2 (7, -7) = (21/2, -21/2).
    The duplicate counts: each copy has its own e row and its own gradient row (1, 0)."""
    x = t64(HAND_X).requires_grad_(True)
    e = t64([[0.5, 1], [-1, -1], [0.5, 1], [-4, 1.5]]).requires_grad_(True)
    src, dst = torch.tensor([0, 1, 0, 1]), torch.tensor([1, 1, 1, 2])
    out = aggregate(x, e, 4, src, dst, 0.5)
    assert torch.equal(out, t64([[1.5, -3], [9.5, 0.75], [-1.5, 8], [10.5, -10.5]]))
    out.sum().backward()
    assert torch.equal(e.grad, t64([[1, 0], [1, 0], [1, 0], [0, 1]]))
    assert torch.equal(x.grad, t64([[3.5, 1.5], [2.5, 2.5], [1.5, 1.5], [1.5, 1.5]]))
    once = aggregate(x, e[1:], 4, src[1:], dst[1:], 0.5)                # the duplicate dropped: one share less
    assert torch.equal((out - once).detach(), t64([[0, 0], [1.5, 0], [0, 0], [0, 0]]))
    conv = RefGINEConv(nn.Identity(), eps=0.5)                          # through the layer: nn sees (1 + eps) x_3
    assert torch.equal(conv(x.detach(), torch.stack([src, dst]), e.detach())[3], t64([10.5, -10.5]))


def test_restatement_exact_tie_has_zero_gradient():
    """0 -> 1 with e = -x_0 = (-1, 2): the relu input is exactly (0, 0), the message 0 and relu'(0) = 0: no gradient
    reaches e, and x_0 gets its root term alone."""
    x = t64(HAND_X[:2]).requires_grad_(True)
    e = t64([[-1, 2]]).requires_grad_(True)
    out = aggregate(x, e, 2, torch.tensor([0]), torch.tensor([1]), 0.5)
    assert torch.equal(out, t64([[1.5, -3], [4.5, 0.75]]))
    out.sum().backward()
    assert torch.equal(e.grad, t64([[0, 0]])) and torch.equal(x.grad, t64([[1.5, 1.5], [1.5, 1.5]]))


def test_restatement_sums_in_either_order():
    case = operator_case(7, "random")
    a, b = run_formula(case, "random"), run_formula(case, "random", reverse=True)
    assert (a[0] - b[0]).abs().max().item() < 1e-12
    assert torch.equal(a[1][1], b[1][1])                                 # g_e is a copy or a zero: no order in it
    assert not torch.equal(run_formula(case, "random", torch.float32)[0],
                           run_formula(case, "random", torch.float32, reverse=True)[0])   # the order is another one


# ---- registry, module layout ------------------------------------------------------------------------------------------

def test_registry():
    from rgb_experiment_amd.dist import experiment as dist_experiment
    from rgb_experiment_amd.initial_params import InitialParameters
    from rgb_experiment_amd.models import MODELS, REGISTRY
    from rgb_experiment_amd import nn as rnn
    assert MODELS["gine"] is GINE and "gine" not in REGISTRY
    assert sorted(REGISTRY) == sorted(["mlp", "gcn", "graphsage", "graphsage2", "gat", "appnpstack", "dagnn", "pta", "sgc",
                                       "gin"])
    assert "gine" not in dist_experiment.SUPPORTED
    assert len(InitialParameters.model_names) == 13
    assert "GINEConv" in rnn.__all__


@pytest.mark.parametrize("with_lin,train_eps", LAYER_FLAGS)
def test_state_dict_layout_and_strict_loading(with_lin, train_eps):
    """PyG's names: nn.*, eps (in the state dict either way: a Parameter or a buffer), lin.* only with edge_dim."""
    from rgb_experiment_amd.nn import Linear
    net = lambda: nn.Sequential(Linear(6, 5), nn.ReLU(), Linear(5, 4))
    conv = GINEConv(net(), eps=0.125, train_eps=train_eps, edge_dim=3 if with_lin else None)
    shapes = {"nn.0.weight": (5, 6), "nn.0.bias": (5,), "nn.2.weight": (4, 5), "nn.2.bias": (4,), "eps": (1,)}
    if with_lin:
        shapes.update({"lin.weight": (6, 3), "lin.bias": (6,)})               # Linear(edge_dim, in_channels), with bias
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == shapes
    assert ("eps" in dict(conv.named_parameters())) == train_eps
    assert conv.eps.item() == 0.125 and conv.in_channels == 6 and (conv.lin is not None) == with_lin
    g = torch.Generator().manual_seed(1)
    state = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    conv.load_state_dict(state, strict=True)
    ref = RefGINEConv(nn.Sequential(nn.Linear(6, 5), nn.ReLU(), nn.Linear(5, 4)).double(), train_eps=train_eps,
                      edge_dim=3 if with_lin else None, in_channels=6)
    ref.load_state_dict({k: v.double() for k, v in conv.state_dict().items()}, strict=True)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    assert sorted(dict(conv.named_parameters())) == sorted(dict(ref.named_parameters()))
    assert all(torch.equal(conv.state_dict()[k], state[k]) for k in state)
    with pytest.raises(RuntimeError):
        conv.load_state_dict({**state, "lin_edge.weight": torch.zeros(6, 3)}, strict=True)


def test_model_layout():
    from rgb_experiment_amd.nn import BatchNorm1d, Linear
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    model = GINE(10, 5, 4, 3, 0.5, 6)
    assert inspect.getfullargspec(GINE.__init__).args[1:] == ["input_dim", "output_dim", "hidden_unit", "num_layers",
                                                              "dropout_rate", "edge_dim"]
    assert inspect.getfullargspec(GINE.forward).args[1:] == ["x", "edge_index", "edge_attr"]
    assert len(model.convs) == 3 and all(isinstance(c, GINEConv) for c in model.convs) and model.dropout_rate == 0.5
    assert isinstance(model.encoder, Linear) and isinstance(model.convs[0].nn[4], BatchNorm1d)
    assert all("eps" in dict(c.named_parameters()) for c in model.convs)      # train_eps=True
    sh = shapes(model)
    assert sh["encoder.weight"] == (4, 10) and sh["convs.0.nn.0.weight"] == (4, 4) and sh["convs.2.nn.2.weight"] == (4, 4)
    assert sh["convs.1.lin.weight"] == (4, 6) and sh["convs.1.lin.bias"] == (4,) and sh["convs.2.eps"] == (1,)
    assert sh["convs.0.nn.4.running_mean"] == (4,) and sh["lin1.weight"] == (4, 4) and sh["lin2.weight"] == (5, 4)
    ref = RefGINE(10, 5, 4, 3, 0.5, 6)
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()},
                        strict=True)
    model.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()},
                          strict=True)
    x, y, ei, ea, model, ref = model_case()
    res = ref(x, ei, ea)
    assert set(res) == {"out", "emb"} and res["out"].shape == (MODEL_SHAPE["n"], MODEL_SHAPE["classes"])


# ---- the slot permutation ------------------------------------------------------------------------------------------

class HostCSR:
    def __init__(self, perm, nnz, N):
        self.perm, self.nnz, self.N = perm, nnz, N


class HostGraph:
    """What ops.edge_rows_to_slots reads of a graph, with the CSR's slot -> edge map built on the host."""

    def __init__(self, name, loops_mode=0):
        ei, n = graph_of(name)
        order = slots_of(name)[3]
        self.N, self.E, self.loops_mode = n, ei.size(1), loops_mode
        self.fwd = HostCSR(order.to(torch.int32), ei.size(1), n)


def host_gather(monkeypatch, calls):
    """ops.gather_rows on the CPU (the HIP kernel's contract: out[r] = src[idx[r]], idx int32), counting its calls."""
    from rgb_experiment_amd import ops

    def gather_rows(src, idx, out=None):
        assert idx.dtype == torch.int32 and src.dim() == 2 and src.is_contiguous()
        calls.append(tuple(src.shape))
        return src.index_select(0, idx.long())
    monkeypatch.setattr(ops, "gather_rows", gather_rows)


def test_edge_rows_to_slots_is_the_permutation_and_is_cached(monkeypatch):
    from rgb_experiment_amd import ops
    calls = []
    host_gather(monkeypatch, calls)
    graph = HostGraph("random")
    order = slots_of("random")[3]
    ea = torch.randn(graph.E, 3, generator=torch.Generator().manual_seed(2))
    got = ops.edge_rows_to_slots(ea, graph)
    assert torch.equal(got, ea[order]) and not got.requires_grad
    assert ops.edge_rows_to_slots(ea, graph) is got and calls == [(graph.E, 3)]       # cached: one gather, at width D
    other = ea.clone()
    assert torch.equal(ops.edge_rows_to_slots(other, graph), got) and len(calls) == 2  # another storage: another entry
    ea.mul_(2.0)                                                                        # in place: the version moves
    assert torch.equal(ops.edge_rows_to_slots(ea, graph), 2 * got) and len(calls) == 3
    empty = HostGraph("no_edges")
    assert ops.edge_rows_to_slots(torch.zeros(0, 3), empty).shape == (0, 3) and len(calls) == 3


def test_edge_rows_to_slots_backward_is_the_inverse_gather(monkeypatch):
    from rgb_experiment_amd import ops
    calls = []
    host_gather(monkeypatch, calls)
    graph = HostGraph("random")
    order = slots_of("random")[3]
    g = torch.Generator().manual_seed(3)
    ea = torch.randn(graph.E, 4, generator=g).requires_grad_(True)
    cot = torch.randn(graph.E, 4, generator=g)
    got = ops.edge_rows_to_slots(ea, graph)
    assert got.requires_grad and torch.equal(got.detach(), ea.detach()[order])
    (got * cot).sum().backward()
    want = torch.empty_like(cot)
    want[order] = cot                                                    # edge order[p] receives slot p's row
    assert torch.equal(ea.grad, want) and len(calls) == 2                # one gather forward, one backward: no scatter
    ops.edge_rows_to_slots(ea, graph)
    assert len(calls) == 3                                               # never cached while it takes a gradient
    assert "_edge_slots" not in graph.__dict__


# ---- refusals ------------------------------------------------------------------------------------------------------

def test_layer_and_operator_refusals():
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, LOOPS_REMOVE_ADD
    x, ei = torch.randn(5, 4), torch.tensor([[0, 1, 2], [1, 2, 3]])
    conv = GINEConv(nn.Sequential(nn.Linear(4, 3)))
    with pytest.raises(ValueError, match="edge_attr"):                   # edge_dim=None: the node width is required
        conv(x, ei, torch.randn(3, 6))
    with pytest.raises(ValueError, match="edge_attr"):
        conv(x, ei, torch.randn(2, 4))                                   # not one row per edge
    with pytest.raises(ValueError, match="edge_attr"):
        conv(x, ei, None)
    lin = GINEConv(nn.Sequential(nn.Linear(4, 3)), edge_dim=6)
    with pytest.raises(ValueError, match="edge_attr"):
        lin(x, ei, torch.randn(3, 4))                                    # edge_dim=6 takes [E, 6]
    with pytest.raises(ValueError, match="first Linear"):
        GINEConv(nn.Sequential(nn.ReLU()), edge_dim=6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(x, ei, torch.randn(3, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lin(x, ei, torch.randn(3, 6))

    class Partitioned:
        is_distributed = True
    t = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="no node-partitioned form"):
        ops.gine_aggregate(t, t, Partitioned())
    with pytest.raises(RuntimeError, match="no node-partitioned form"):
        ops.edge_rows_to_slots(t, Partitioned())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gine_aggregate(t, t, object())
    for mode in (LOOPS_ADD_REMAINING, LOOPS_REMOVE_ADD):
        graph = HostGraph("random", loops_mode=mode)
        with pytest.raises(RuntimeError, match="LOOPS_KEEP"):
            ops.edge_rows_to_slots(torch.zeros(graph.E, 3), graph)
    graph = HostGraph("random")
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.edge_rows_to_slots(torch.zeros(graph.E - 1, 3), graph)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.edge_rows_to_slots(torch.zeros(graph.E, 3), graph)            # a CPU tensor reaches the gather and is refused


class EdgeModel(nn.Module):
    """A caller's module whose forward takes edge_attr (dense work only: it runs on the CPU)."""

    def __init__(self, f, d, c):
        super().__init__()
        self.lin, self.edge = nn.Linear(f, c), nn.Linear(d, c)
        self.seen = None

    def forward(self, x, edge_index, edge_attr):
        self.seen = edge_attr
        h = self.lin(x) + self.edge(edge_attr).mean(0)
        return {"out": F.log_softmax(h, dim=1), "emb": h}


class PlainModel(nn.Module):
    def __init__(self, f, c):
        super().__init__()
        self.lin = nn.Linear(f, c)

    def forward(self, x, edge_index):
        h = self.lin(x)
        return {"out": F.log_softmax(h, dim=1), "emb": h}


def _data(with_attr, attr=None):
    from rgb_experiment_amd.data import Data
    g = torch.Generator().manual_seed(5)
    n = 60
    extra = {}
    if with_attr:
        extra["edge_attr"] = torch.randn(300, 4, generator=torch.Generator().manual_seed(6)) if attr is None else attr
    return Data(x=torch.randn(n, 8, generator=g), y=torch.randint(0, 3, (n,), generator=g),
                edge_index=torch.randint(0, n, (2, 300), generator=g), **extra)


def _run(data, **kw):
    from rgb_experiment_amd import experiment
    args = dict(specify_data=True, data=data, remake_data_mask=True, epoch=4, print_print=False, return_model=True,
                need_to_reappear=True, use_cpu=True, model_name="mlp")
    args.update(kw)
    init = args.pop("init", {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.5})
    return experiment(init, **args)


GINE_INIT = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0, "edge_dim": 4}


def test_experiment_refusals():
    sig = inspect.signature(__import__("rgb_experiment_amd").experiment).parameters
    assert sig["use_edge_attr"].default is False
    for name in ("mlp", "gcn", "graphsage", "gat", "gin", "dagnn", "resgated", "transformer"):
        with pytest.raises(ValueError, match="takes no edge attributes"):
            _run(_data(True), model_name=name, use_edge_attr=True)
    with pytest.raises(ValueError, match="takes no edge_attr"):
        _run(_data(True), model=PlainModel(8, 3), use_edge_attr=True)
    with pytest.raises(ValueError, match="to_undirected"):
        _run(_data(True), model_name="gine", init=GINE_INIT, use_edge_attr=True, to_undirected_graph=True)
    with pytest.raises(NotImplementedError, match="partitioned"):
        _run(_data(True), model_name="gine", init=GINE_INIT, use_edge_attr=True, distributed=True)
    with pytest.raises(NotImplementedError):  # the name checks stay in front
        _run(_data(True), model_name="fagcn", use_edge_attr=True)
    with pytest.raises(ValueError, match="unknown model_name"):
        _run(_data(True), model_name="nonesuch", use_edge_attr=True)
    with pytest.raises(NotImplementedError):
        _run(_data(True), model_name="gine", init=GINE_INIT, use_edge_attr=True, print_pics=True)
    # data.edge_attr must be float [E, D]
    with pytest.raises(ValueError, match="needs data.edge_attr"):
        _run(_data(False), model_name="gine", init=GINE_INIT, use_edge_attr=True)
    with pytest.raises(ValueError, match="needs data.edge_attr"):
        _run(_data(True, torch.zeros(300, 4, dtype=torch.int64)), model_name="gine", init=GINE_INIT, use_edge_attr=True)
    with pytest.raises(ValueError, match=r"\[E, D\]"):
        _run(_data(True, torch.zeros(300)), model_name="gine", init=GINE_INIT, use_edge_attr=True)
    with pytest.raises(ValueError, match=r"\[E, D\]"):
        _run(_data(True, torch.zeros(299, 4)), model_name="gine", init=GINE_INIT, use_edge_attr=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # well-formed: the device check is next
        _run(_data(True), model_name="gine", init=GINE_INIT, use_edge_attr=True)


def test_a_callers_model_receives_edge_attr():
    data = _data(True)
    model = EdgeModel(8, 4, 3)
    before = copy.deepcopy(model.edge.weight.detach())
    res = _run(data, model=model, use_edge_attr=True)
    assert model.seen is not None and model.seen.dtype == torch.float32 and torch.equal(model.seen, data.edge_attr)
    assert len(res["history"]["train_loss"]) == 4 and not torch.equal(model.edge.weight.detach(), before)
    with pytest.raises(TypeError):                                       # flag off: the argument is not passed
        _run(data, model=EdgeModel(8, 4, 3))


def test_an_unused_edge_attr_attribute_changes_nothing():
    a = _run(_data(False))
    b = _run(_data(True))
    assert a["history"] == b["history"]
    assert a["ACC"] == b["ACC"]
    plain = lambda: (torch.manual_seed(3), PlainModel(8, 3))[1]
    c = _run(_data(False), model=plain())
    d = _run(_data(True), model=plain())
    assert c["history"] == d["history"]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

NEW_ENTRIES = ("rgbx_gine_supported", "rgbx_gine_fwd_f32", "rgbx_gine_bwd_edge_f32", "rgbx_gine_bwd_src_f32")


def test_abi_declares_and_exports_the_new_entries():
    from rgb_experiment_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbx_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rgbx_[a-z0-9_]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS, name
        params = re.search(name + r"\s*\(([^)]*)\)", text).group(1)       # one ctypes argument per declared parameter
        assert len(_lib.SIGNATURES[name]) == len([a for a in params.split(",") if a.strip()]), name
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.rgbx_version() == 501
    for C in range(1, 301):
        assert bool(lib.rgbx_gine_supported(C)) == bool(lib.rgbx_transformer_supported(1, C)), C
    assert not lib.rgbx_gine_supported(0) and not lib.rgbx_gine_supported(-4)
    assert all(lib.rgbx_gine_supported(C) for C in WIDTHS)
    assert not any(lib.rgbx_gine_supported(C) for C in (67, 130, 260, BLOCKED_WIDTH))
    p = 0x10000  # 16-byte aligned, non-null, never dereferenced: every call below returns before a launch

    def fwd(**kw):
        a = dict(rowptr=p, col=p, x=p, ldx=64, e=p, lde=64, eps=p, out=p, ldo=64, N=10, C=64)
        a.update(kw)
        return lib.rgbx_gine_fwd_f32(a["rowptr"], a["col"], a["x"], a["ldx"], a["e"], a["lde"], a["eps"], a["out"],
                                     a["ldo"], a["N"], a["C"], None, None)
    assert fwd(rowptr=None) == -1 and b"null" in lib.rgbx_last_error_string()
    assert fwd(col=None) == -1 and fwd(x=None) == -1 and fwd(e=None) == -1 and fwd(out=None) == -1
    assert fwd(ldx=63) == -1 and b"leading dimension" in lib.rgbx_last_error_string()
    assert fwd(lde=32) == -1 and fwd(ldo=8) == -1
    assert fwd(N=-1) == -1 and fwd(C=0) == -1
    assert fwd(N=2 ** 31) == -2                                           # RGBX_E_RANGE
    assert fwd(C=67, ldx=67, lde=67, ldo=67) == -5                        # RGBX_E_SHAPE
    assert fwd(C=130, ldx=130, lde=130, ldo=130) == -5 and fwd(C=1000) == -5
    assert fwd(e=p + 2) == -3 and b"aligned" in lib.rgbx_last_error_string()   # RGBX_E_ALIGN
    assert fwd(x=p + 1) == -3 and fwd(out=p + 3) == -3 and fwd(eps=p + 2) == -3
    # C = 256 needs 4 floats per lane: 16-byte pointers and leading dimensions that are multiples of 4
    wide = dict(C=256, ldx=256, lde=256, ldo=256)
    assert fwd(**{**wide, "e": p + 8}) == -5 and b"lanes" in lib.rgbx_last_error_string()
    assert fwd(**{**wide, "lde": 258}) == -5
    assert fwd(N=0) == 0 and fwd(N=0, rowptr=None) == 0                   # nothing to do

    def edge(**kw):
        a = dict(x=p, e=p, gout=p, ldg=64, g_e=p, ldge=64, N=1000, C=64)
        a.update(kw)
        return lib.rgbx_gine_bwd_edge_f32(p, p, a["x"], 64, a["e"], 64, a["gout"], a["ldg"], a["g_e"], a["ldge"], a["N"],
                                          a["C"], None, None)
    assert edge(x=None) == -1 and edge(e=None) == -1 and edge(gout=None) == -1 and edge(g_e=None) == -1
    assert edge(ldg=32) == -1 and edge(ldge=63) == -1
    assert edge(gout=p + 2) == -3 and edge(g_e=p + 1) == -3
    assert edge(C=67) == -5
    assert edge(N=2 ** 31) == -2 and edge(N=0) == 0

    def src(**kw):
        a = dict(t2f=p, x=p, e=p, gout=p, eps=p, g_x=p, ldgx=64, N=1000, C=64)
        a.update(kw)
        return lib.rgbx_gine_bwd_src_f32(p, p, a["t2f"], a["x"], 64, a["e"], 64, a["gout"], 64, a["eps"], a["g_x"],
                                         a["ldgx"], a["N"], a["C"], None, None)
    assert src(t2f=None) == -1 and src(x=None) == -1 and src(e=None) == -1 and src(gout=None) == -1
    assert src(g_x=None) == -1
    assert src(ldgx=63) == -1
    assert src(g_x=p + 2) == -3 and src(e=p + 1) == -3 and src(eps=p + 1) == -3
    assert src(C=130) == -5
    assert src(N=2 ** 31) == -2 and src(N=0) == 0


# ---- preconditions of the GPU cases ----------------------------------------------------------------------------------

def test_widths_cover_the_layout():
    """(vector width, lanes per row) over WIDTHS, as attn_common.h's pick_vec / make_layout choose them on aligned rows:
    all three vector widths and every group count from 64 rows per wave-instruction down to 1."""
    pow2ceil = lambda x: 1 << (x - 1).bit_length()
    seen = set()
    for C in WIDTHS:
        vec = 4 if C % 4 == 0 else (2 if C % 2 == 0 else 1)
        seen.add((vec, 64 // pow2ceil(-(-C // vec))))
    assert {v for v, _ in seen} == {1, 2, 4}
    assert {ng for _, ng in seen} >= {64, 8, 4, 2, 1}
    assert {4 if C % 4 == 0 else (2 if C % 2 == 0 else 1) for C in DEGREE_WIDTHS} == {1, 2, 4}


def test_graphs_have_what_the_cases_need():
    from rgb_experiment_amd.graph import LONG_ROW_SLOTS as product_threshold
    assert LONG_ROW_SLOTS == product_threshold
    ei, n = graph_of("degrees")
    indeg, outdeg = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
    assert tuple(indeg[:6].tolist()) == DEGREES and tuple(outdeg[6:12].tolist()) == DEGREES
    assert DEGREES == (0, 1, 64, 65, 1024, 1025)
    ei, n = graph_of("powerlaw")
    assert int(torch.bincount(ei[1], minlength=n).max()) > LONG_ROW_SLOTS     # hub rows in both CSRs
    assert int(torch.bincount(ei[0], minlength=n).max()) > LONG_ROW_SLOTS
    ei, n = graph_of("random")
    indeg, outdeg = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
    assert bool((indeg[:20] == 0).all()) and bool((outdeg[20:40] == 0).all())
    assert int((ei[0] == ei[1]).sum()) > 0 and torch.unique(ei[0] * n + ei[1]).numel() < ei.size(1)
    assert [graph_of(name)[1] for name in SMALL_GRAPHS] == [1, 2, 3]
    for name in SMALL_GRAPHS:
        ei, n = graph_of(name)
        assert int((ei[0] == ei[1]).sum()) > 0 and torch.unique(ei[0] * n + ei[1]).numel() < ei.size(1)


OPERATOR_CASES = ([(C, g) for C in WIDTHS for g in GRAPH_NAMES] + [(C, "degrees") for C in DEGREE_WIDTHS]
                  + [(C, g) for C in SMALL_WIDTHS for g in SMALL_GRAPHS] + [(BLOCKED_WIDTH, "random")])


@pytest.mark.parametrize("C,graph", OPERATOR_CASES)
def test_operator_case_is_well_posed(C, graph):
    case = operator_case(C, graph)
    assert all(torch.equal(t, t.float().double()) for t in case)              # exactly representable in float32
    ties = check_masks_agree(case, graph)
    want = reference(C, graph)
    low = run_formula(case, graph, torch.float32, reverse=True)
    shares = shares_of(low, want)
    print(f"C = {C} {graph}: {ties} planted ties, max |out| {want[0].abs().max().item():.1f}; float32 (reversed order) vs "
          f"float64 share of tolerance {shares}")
    assert all(torch.isfinite(t).all() for t in [low[0]] + low[1])
    assert max(shares.values()) <= WELL_POSED_SHARE, shares
    assert torch.equal(low[1][1].double(), want[1][1])                        # g_e: the same mask, the same copies
    ei, n = graph_of(graph)
    assert ties == len(range(0, ei.size(1), TIE_EVERY))
    k, c = tie_positions(ei.size(1), C)
    assert want[1][1][k, c].abs().max().item() == 0.0 if ties else True       # relu'(0) = 0
    x, cot = case[0], case[2]
    if graph == "no_edges":
        assert torch.equal(want[0], (1 + EPS) * x) and torch.equal(want[1][0], (1 + EPS) * cot)
    if graph == "random":      # rows without in-edges / sources without out-edges: the root term alone
        assert torch.equal(want[0][:20], (1 + EPS) * x[:20]) and torch.equal(want[1][0][20:40], (1 + EPS) * cot[20:40])
    if graph == "powerlaw":    # the hub rows grow with the degree
        hub = int(torch.bincount(ei[1], minlength=n).argmax())
        assert want[0][hub].abs().max().item() > 10.0


@pytest.mark.parametrize("with_lin,train_eps", LAYER_FLAGS)
@pytest.mark.parametrize("C", LAYER_WIDTHS)
def test_layer_case_is_well_posed(C, with_lin, train_eps):
    x, ei, ea, ref = layer_case(C, with_lin, train_eps)
    cot = f32_exact((LAYER_N, 5), torch.Generator().manual_seed(17))
    low = copy.deepcopy(ref).float()
    x64, x32 = x.clone().requires_grad_(True), x.float().requires_grad_(True)
    ea64, ea32 = ea.clone().requires_grad_(True), ea.float().requires_grad_(True)
    want, got = ref(x64, ei, ea64), low(x32, ei, ea32, reverse=True)
    margin = relu_margin(ref, x, ei, ea)
    z = ref.relu_inputs
    print(f"C = {C} edge_dim={'set' if with_lin else None}: min |relu input| {z.abs().min().item():.3e}, largest margin "
          f"{margin.max().item():.3e}, smallest |relu input| / margin {(z.abs() / margin).min().item():.1f}")
    assert bool((z.abs() > margin).all()), "a relu input of the reference lies within float32's reach of zero"
    assert torch.equal(low.relu_inputs > 0, z > 0)
    (want * cot).sum().backward()
    (got * cot.float()).sum().backward()
    shares = {"forward": share_of_tolerance(got, want, FWD_TOL), "x": share_of_tolerance(x32.grad, x64.grad, GRAD_TOL),
              "edge_attr": share_of_tolerance(ea32.grad, ea64.grad, GRAD_TOL)}
    lowp = dict(low.named_parameters())
    for key, prm in ref.named_parameters():
        shares[key] = share_of_tolerance(lowp[key].grad, prm.grad, GRAD_TOL)
    print(shares)
    assert len(shares) == 3 + 4 + 2 * with_lin + train_eps
    assert max(shares.values()) <= WELL_POSED_SHARE, shares
    assert int((torch.bincount(ei[1], minlength=LAYER_N) == 0).sum()) > 0   # nodes without in-edges


def model_margins(ref, low, x, ei, ea):
    """Per conv, the relu-input margin of the reference model after one forward of `ref` (float64) and `low` (its float32
    copy, edges reversed). The conv's input h is itself the output of float32 layers — the encoder's product for the first
    conv; two products, two relus and BatchNorm's affine map of the previous block for the others — so it arrives with an
    error. That error is bounded from the reference alone: four times the deviation of the float32 reference run from
    the float64 one (the GPU sums in another order than either: a factor of two on the deviation for the order, two for
    safety), plus BatchNorm's own rounding, (v - mean) * rstd * weight + bias in float32: three roundings of a value of
    size |h| + |bias|, 3 u (|h| + |bias|)."""
    out = []
    for k, conv in enumerate(ref.convs):
        h64, h32 = ref.conv_inputs[k], low.conv_inputs[k].double()
        x_err = 4 * (h32 - h64).abs().max().item()
        if k > 0:
            bn = ref.convs[k - 1].nn[4]
            x_err = x_err + 3 * U32 * (h64.abs() + bn.bias.detach().abs())
        out.append(relu_margin(conv, h64, ei, ea, x_err))
    return out


def test_model_case_is_well_posed():
    x, y, ei, ea, model, ref = model_case()
    ref.train()
    low = copy.deepcopy(ref).float()
    want, got = ref(x, ei, ea), low(x.float(), ei, ea.float(), reverse=True)
    for k, margin in enumerate(model_margins(ref, low, x, ei, ea)):
        z = ref.convs[k].relu_inputs
        print(f"conv {k}: min |relu input| {z.abs().min().item():.3e}, largest margin {margin.max().item():.3e}, smallest "
              f"|relu input| / margin {(z.abs() / margin).min().item():.1f}")
        assert bool((z.abs() > margin).all()), f"conv {k}: a relu input lies within float32's reach of zero"
        assert torch.equal(low.convs[k].relu_inputs > 0, z > 0)
    F.nll_loss(want["out"], y).backward()
    F.nll_loss(got["out"], y).backward()
    shares = {"emb": share_of_tolerance(got["emb"], want["emb"], FWD_TOL),
              "out": share_of_tolerance(got["out"], want["out"], FWD_TOL)}
    lowp = dict(low.named_parameters())
    for key, prm in ref.named_parameters():
        shares[key] = share_of_tolerance(lowp[key].grad, prm.grad, GRAD_TOL)
    print(shares)
    assert any(k.endswith("eps") for k in shares) and any(k.endswith("lin.weight") for k in shares)
    assert max(shares.values()) <= WELL_POSED_SHARE, shares
