"""GMMConv / MoNet on the host: a float64 restatement of the layer written the way PyG's `message` is (a broadcast
[E, K, D] difference, the Gaussians of every edge, the messages added per target with index_add and divided by a bincount),
not with CSR slots as the product computes it; pinned by numbers derived by hand. Registry, module layout (PyG's names,
strict state_dict loading both ways), refusals, experiment(model_name="monet") on the CPU up to the device check, the C ABI
of the new entry points, the degree pseudo-coordinates restated; and the case builders tests/test_gpu_gmm.py feeds to the
HIP kernels, with the checks that keep those cases well-posed. No GPU needed.

Well-posedness. The inputs are exactly representable in float32: e and mu in [0, 1]^D, |sigma| in [0.5, 1.5] with both
signs (so no Gaussian underflows, the exponent stays above -0.5 * 8 * 4 = -16 and the 1e-15 in the denominator is
immaterial), h, y0 and the cotangent N(0, 1). What separates float32 from float64 is then rounding in the exponent and in
the sums: every case is run through the restatement in float32 on the CPU with the edges and the kernels in REVERSED order
and has to stay within a QUARTER (WELL_POSED_SHARE) of the GPU test's tolerances (forward 1e-4, gradients 2e-4, times
max(1, |ref|max)) of the float64 result. Seeds are fixed; a case that does not satisfy this fails, it is never skipped."""
import copy
import ctypes
import functools
import inspect
import math
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from rgb_experiment_amd.models import MoNet            # without the feature this file fails here, at import
from rgb_experiment_amd.nn import GMMConv

import test_gine_host as G
from test_transformer_host import FWD_TOL, GRAD_TOL, LONG_ROW_SLOTS, WELL_POSED_SHARE, f32_exact, share_of_tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-15


# ---- the restatement ---------------------------------------------------------------------------------------------------

def gaussians(e, mu, sigma):
    """[E, K] from e [E, D] and mu, sigma [K, D]: PyG's GMMConv.message, separate_gaussians=False."""
    E, D = e.shape
    K = mu.size(0)
    g = -0.5 * (e.view(E, 1, D) - mu.view(1, K, D)).pow(2)
    g = g / (EPS + sigma.view(1, K, D).pow(2))
    return torch.exp(g.sum(dim=-1))


def aggregate(h, e, mu, sigma, n, src, dst, aggr="mean", reverse=False):
    """out [n, M]: per edge (src -> dst), as given, the message sum_k gauss[edge, k] * h[src].view(K, M)[k], added per
    target; aggr="mean" divides by the number of in-edges, duplicates counted. e holds one row per INPUT edge. `reverse`:
    edges and kernels backwards."""
    K = mu.size(0)
    M = h.size(1) // K
    if reverse:
        src, dst, e = src.flip(0), dst.flip(0), e.flip(0)
    E = src.numel()
    weighted = h.index_select(0, src).view(E, K, M) * gaussians(e, mu, sigma).view(E, K, 1)
    msg = weighted.flip(1).sum(dim=-2) if reverse else weighted.sum(dim=-2)
    out = torch.zeros(n, M, dtype=h.dtype).index_add(0, dst, msg)
    if aggr == "mean":
        out = out / torch.bincount(dst, minlength=n).clamp(min=1).to(h.dtype)[:, None]
    elif aggr not in ("add", "sum"):
        raise ValueError(aggr)
    return out


def degree_pseudo(ei, n):
    """float32 [E, 2], one row per INPUT edge: (1 / sqrt(1 + indeg(src)), 1 / sqrt(1 + indeg(dst))), the in-degrees as given:
    one CORRECTLY ROUNDED float32 square root and one correctly rounded float32 division of exact integers, which is what
    IEEE 754 asks of both and what the kernel computes. Each is taken in float64 and rounded to float32: for a square root
    and for a quotient of float32 values 53 >= 2 * 24 + 2 bits make the second rounding innocuous. (torch's vectorised
    float32 sqrt on the CPU is NOT always correctly rounded, sqrt(267.0f) for one, so it is not used.)"""
    deg = torch.bincount(ei[1], minlength=n)
    root = torch.sqrt((1 + deg).to(torch.float64)).to(torch.float32)
    r = (1.0 / root.to(torch.float64)).to(torch.float32)
    return torch.stack([r[ei[0]], r[ei[1]]], dim=1)


class RefGMMConv(nn.Module):
    """float64 restatement of GMMConv with PyG's parameter names and shapes: g [in, out * K], mu, sigma [K, dim],
    root.weight [out, in] with root_weight, bias [out]."""

    def __init__(self, in_channels, out_channels, dim, kernel_size, aggr="mean", root_weight=True, bias=True):
        super().__init__()
        self.aggr = aggr
        f64 = lambda *shape: nn.Parameter(torch.zeros(*shape, dtype=torch.float64))
        self.g = f64(in_channels, out_channels * kernel_size)
        self.mu, self.sigma = f64(kernel_size, dim), f64(kernel_size, dim)
        self.root = nn.Linear(in_channels, out_channels, bias=False, dtype=torch.float64) if root_weight else None
        self.bias = f64(out_channels) if bias else None

    def forward(self, x, ei, ea, reverse=False):
        out = aggregate(x @ self.g, ea, self.mu, self.sigma, x.size(0), ei[0], ei[1], self.aggr, reverse)
        if self.root is not None:
            out = out + self.root(x)
        if self.bias is not None:
            out = out + self.bias
        return out


class RefMoNet(nn.Module):
    """models/monet.py in float64: num_layers GMMConv layers, ELU and dropout between them; the product's names."""

    def __init__(self, input_dim, output_dim, hidden_unit, num_layers, dropout_rate, kernel_size, dim=2):
        super().__init__()
        self.dropout_rate = dropout_rate
        dims = [input_dim] + [hidden_unit] * (num_layers - 1) + [output_dim]
        self.convs = nn.ModuleList(RefGMMConv(a, b, dim, kernel_size) for a, b in zip(dims[:-1], dims[1:]))

    def forward(self, x, ei, ea=None, reverse=False):
        if ea is None:
            ea = degree_pseudo(ei, x.size(0)).to(x.dtype)
        for i, conv in enumerate(self.convs):
            x = conv(x, ei, ea, reverse)
            if i + 1 < len(self.convs):
                x = F.dropout(F.elu(x), p=self.dropout_rate, training=self.training)
        return {"out": F.log_softmax(x, dim=1), "emb": x}


def unit_coords(shape, gen):
    """float64 values in [0, 1) that are exactly representable in float32."""
    return torch.rand(shape, generator=gen).double()


def spread_sigma(shape, gen):
    """float64, fp32-exact, |sigma| in [0.5, 1.5) with both signs."""
    mag = 0.5 + torch.rand(shape, generator=gen)
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)
    return (mag * sign).double()


def randomize(module, seed):
    """Every parameter of a reference module set to fp32-exact values: N(0, 0.5), but mu in [0, 1) and |sigma| in
    [0.5, 1.5) with both signs."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            leaf = name.rsplit(".", 1)[-1]
            if leaf == "mu":
                p.copy_(unit_coords(tuple(p.shape), g))
            elif leaf == "sigma":
                p.copy_(spread_sigma(tuple(p.shape), g))
            else:
                p.copy_(f32_exact(tuple(p.shape), g, 0.5))
    return module


# ---- graphs ---------------------------------------------------------------------------------------------------------

graph_names = ("no_edges", "random", "powerlaw", "degrees") + G.SMALL_GRAPHS
PLANTED_MU = (0.5, 0.25)


@functools.lru_cache(maxsize=None)
def graph_of(name):
    """tests/test_gine_host.graph_of, plus `planted`: 6 nodes. Target 0: the edges 1 -> 0 and 2 -> 0, both exactly on mu_0.
    Target 1: the edge 3 -> 1 at distance 1 from mu_0 along the first coordinate. Target 2: the edge 4 -> 2 twice (a
    duplicate) at distance 1 along the second coordinate, and the self-loop 2 -> 2 on mu_0. Nodes 3, 4 and 5 have no
    in-edge."""
    if name == "planted":
        return torch.tensor([[1, 2, 3, 4, 4, 2], [0, 0, 1, 2, 2, 2]]), 6
    return G.graph_of(name)


@functools.lru_cache(maxsize=None)
def slots_of(name):
    if name == "planted":
        ei, n = graph_of(name)
        order = torch.argsort(ei[1], stable=True)
        rowptr = torch.zeros(n + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(torch.bincount(ei[1], minlength=n), 0)
        return ei[0], ei[1], rowptr, order
    return G.slots_of(name)


def planted_case():
    """(h [6, 1], e [6, 2], mu [1, 2], sigma [1, 2]) in float64: one kernel, one channel, sigma = 1 (one of them -1: only
    its square enters), h_j = j + 1, so every number is scalar arithmetic."""
    m0, m1 = PLANTED_MU
    e = torch.tensor([[m0, m1], [m0, m1], [m0 + 1.0, m1], [m0, m1 + 1.0], [m0, m1 - 1.0], [m0, m1]], dtype=torch.float64)
    h = torch.arange(1, 7, dtype=torch.float64)[:, None]
    return h, e, torch.tensor([[m0, m1]], dtype=torch.float64), torch.tensor([[1.0, -1.0]], dtype=torch.float64)


def planted_expected(aggr):
    """target 0: gauss = 1 twice, (2 + 3) / 2. target 1: 4 exp(-1/2). target 2: (5 exp(-1/2) + 5 exp(-1/2) + 3) / 3, the
    self-loop on mu_0 with coefficient 1. Nodes 3 .. 5: no in-edge, zeros. The sum drops the divisions."""
    a = math.exp(-0.5)
    if aggr == "mean":
        return [2.5, 4 * a, (10 * a + 3) / 3, 0.0, 0.0, 0.0]
    return [5.0, 4 * a, 10 * a + 3, 0.0, 0.0, 0.0]


# ---- operator cases shared with tests/test_gpu_gmm.py ----------------------------------------------------------------

# (K, M): vector widths 1 (7, 5), 2 (66) and 4 (4, 16, 40, 64, 256); the heads in one chunk ((1, 4), (1, 7), (3, 5),
# (8, 16), (4, 64)) and in several ((2, 66), (8, 40)); one head on all 64 lanes (1, 256).
PAIRS = [(1, 4), (1, 7), (3, 5), (2, 66), (8, 16), (8, 40), (4, 64), (1, 256)]
DIMS = [1, 2, 3, 8]
SWEEP_PAIRS = [(3, 5), (2, 66), (8, 16)]             # one pair per vector width, for the sweep over the graphs
# (K, M, D, graph, aggr, with_y0)
CASES = ([(K, M, DIMS[i % 4], "random", "mean", True) for i, (K, M) in enumerate(PAIRS)]
         + [(K, M, DIMS[(i + 1) % 4], "degrees", "sum" if i % 2 else "mean", i % 2 == 0) for i, (K, M) in enumerate(PAIRS)]
         + [(K, M, 2, g, "mean", True) for K, M in SWEEP_PAIRS for g in graph_names if g not in ("random",)]
         + [(8, 16, D, "powerlaw", "sum", False) for D in DIMS]
         + [(4, 64, 3, "random", "add", False), (1, 256, 8, "random", "sum", True), (3, 5, 8, "n3", "sum", False)])
NAMES = ("forward", "g_h", "g_e", "g_mu", "g_sigma", "g_y0")


@functools.lru_cache(maxsize=4)
def operator_case(K, M, D, graph_name):
    """h [n, K * M], e [E, D] (one row per INPUT edge), mu, sigma [K, D], y0 and the cotangent [n, M]: float64, fp32-exact."""
    ei, n = graph_of(graph_name)
    g = torch.Generator().manual_seed(11000 + 1000 * D + 10 * K + M)
    return (f32_exact((n, K * M), g), unit_coords((ei.size(1), D), g), unit_coords((K, D), g), spread_sigma((K, D), g),
            f32_exact((n, M), g), f32_exact((n, M), g))


def run_formula(case, graph_name, aggr, with_y0=True, dtype=torch.float64, reverse=False):
    """The restatement on a case in `dtype`: (out, [g_h, g_e, g_mu, g_sigma, g_y0]); g_e per INPUT edge."""
    ei, n = graph_of(graph_name)
    h, e, mu, sigma, y0 = (t.to(dtype).clone().requires_grad_(True) for t in case[:5])
    out = aggregate(h, e, mu, sigma, n, ei[0], ei[1], aggr, reverse)
    if with_y0:
        out = out + y0
    (out * case[5].to(dtype)).sum().backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return out.detach(), [zero(h), zero(e), zero(mu), zero(sigma), y0.grad if with_y0 else None]


@functools.lru_cache(maxsize=4)
def reference(K, M, D, graph_name, aggr, with_y0):
    """The float64 result of a case, computed once and shared (read-only) by the host and the GPU tests."""
    return run_formula(operator_case(K, M, D, graph_name), graph_name, "add" if aggr == "sum" else aggr, with_y0)


def shares_of(got, want):
    out = {NAMES[0]: share_of_tolerance(got[0], want[0], FWD_TOL)}
    for name, a, b in zip(NAMES[1:], got[1], want[1]):
        if b is None:
            assert a is None
            continue
        assert a.shape == b.shape, name
        if b.numel():                                                     # g_e of a graph without edges: [0, D]
            out[name] = share_of_tolerance(a, b, GRAD_TOL)
    return out


# ---- the seeded differential fuzz of tests/test_gpu_gmm.py ----------------------------------------------------------------

FUZZ_SEEDS = list(range(24))
FUZZ_MAX_WIDTH = 512                  # K * M: the restatement's [E, K, M] tensor stays below 100 MB in float64
FUZZ_MIN_NODES = 31                   # below it a star of thousands of slots is one edge repeated: see fuzz_case


@functools.lru_cache(maxsize=2)
def fuzz_case(seed):
    """A case drawn from the lists of tests/test_gpu_fuzz_families.py (imported, not edited): K from HEADS, M from
    CHANNELS (redrawn until K * M <= FUZZ_MAX_WIDTH), n from NODES, a few targets and sources with exact degrees from
    DEGREES; D from 1 .. 8, aggr and y0 by coin. Graphs of fewer than 31 nodes are left to the operator cases (n1 .. n3):
    with them a row of thousands of slots repeats ONE edge, and a float32 accumulator that adds one value m times drifts
    by m 2^-25 of the sum in any order of summation, the CPU's included, which says nothing about a kernel.
    Returns (K, M, D, aggr, with_y0, edge_index, n, tensors as operator_case gives them)."""
    import random
    import test_gpu_fuzz_families as FF
    from rgb_experiment_amd.graph import LOOPS_KEEP
    rng = random.Random(770000 + seed)
    K = rng.choice(FF.HEADS)
    M = rng.choice(FF.CHANNELS)
    while K * M > FUZZ_MAX_WIDTH:
        M = rng.choice(FF.CHANNELS)
    D = rng.randrange(1, 9)
    n = rng.choice([v for v in FF.NODES if v >= FUZZ_MIN_NODES])
    ei, din, dout = FF.prescribed_graph(rng, n, LOOPS_KEEP)
    aggr, with_y0 = rng.choice(["mean", "sum"]), rng.random() < 0.5
    g = torch.Generator().manual_seed(880000 + seed)
    tensors = (f32_exact((n, K * M), g), unit_coords((ei.size(1), D), g), unit_coords((K, D), g), spread_sigma((K, D), g),
               f32_exact((n, M), g), f32_exact((n, M), g))
    return K, M, D, aggr, with_y0, ei.contiguous(), n, tensors


def run_fuzz(seed, dtype=torch.float64, reverse=False):
    K, M, D, aggr, with_y0, ei, n, case = fuzz_case(seed)
    h, e, mu, sigma, y0 = (t.to(dtype).clone().requires_grad_(True) for t in case[:5])
    out = aggregate(h, e, mu, sigma, n, ei[0], ei[1], "add" if aggr == "sum" else aggr, reverse)
    if with_y0:
        out = out + y0
    (out * case[5].to(dtype)).sum().backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return out.detach(), [zero(h), zero(e), zero(mu), zero(sigma), y0.grad if with_y0 else None]


# ---- layer and model cases ----------------------------------------------------------------------------------------------

PADDED_WIDTH = 67                     # outside the layout: the layer pads it to 68
LAYER_N, LAYER_E, LAYER_F = 80, 500, 6
LAYER_CASES = {   # name -> (out_channels, dim, kernel_size, layer keywords)
    "plain": (7, 2, 3, dict()),
    "padded": (PADDED_WIDTH, 2, 3, dict()),
    "add": (7, 3, 2, dict(aggr="add")),
    "sum_no_root": (16, 1, 5, dict(aggr="sum", root_weight=False)),
    "no_bias": (16, 8, 2, dict(bias=False)),
    "bare": (5, 2, 1, dict(root_weight=False, bias=False)),
}


def layer_case(name):
    """(x float64 fp32-exact, edge_index, edge_attr float64 fp32-exact in [0, 1), reference layer with random parameters)."""
    from test_gpu_ggnn import rand_graph
    M, D, K, kw = LAYER_CASES[name]
    ei = rand_graph(LAYER_N, LAYER_E, 41, loops=5, dups=12)
    g = torch.Generator().manual_seed(43)
    x, ea = f32_exact((LAYER_N, LAYER_F), g), unit_coords((ei.size(1), D), g)
    return x, ei, ea, randomize(RefGMMConv(LAYER_F, M, D, K, **kw), 44)


MODEL_SHAPE = dict(n=60, e=300, f=16, hidden=12, classes=5, layers=3, kernels=3, dim=2)


def model_case():
    """(x, y, edge_index, edge_attr, the product's model on the CPU, the reference holding the same parameters)."""
    from test_gpu_ggnn import rand_graph
    s = MODEL_SHAPE
    g = torch.Generator().manual_seed(51)
    ei = rand_graph(s["n"], s["e"], 52, loops=4, dups=6)
    x, y = f32_exact((s["n"], s["f"]), g), torch.randint(0, s["classes"], (s["n"],), generator=g)
    ea = unit_coords((ei.size(1), s["dim"]), g)
    ref = randomize(RefMoNet(s["f"], s["classes"], s["hidden"], s["layers"], 0.0, s["kernels"], s["dim"]), 53)
    model = MoNet(s["f"], s["classes"], s["hidden"], s["layers"], 0.0, s["kernels"], s["dim"])
    model.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return x, y, ei, ea, model, ref


# ---- the restatement, pinned ------------------------------------------------------------------------------------------

def test_restatement_reproduces_hand_computed_numbers():
    ei, n = graph_of("planted")
    h, e, mu, sigma = planted_case()
    assert gaussians(e, mu, sigma).flatten().tolist() == pytest.approx(
        [1.0, 1.0, math.exp(-0.5), math.exp(-0.5), math.exp(-0.5), 1.0], rel=0, abs=1e-15)
    for aggr in ("mean", "add", "sum"):
        got = aggregate(h, e, mu, sigma, n, ei[0], ei[1], aggr).flatten().tolist()
        assert got == pytest.approx(planted_expected(aggr), rel=0, abs=1e-12), aggr
    assert got[3:] == [0.0, 0.0, 0.0]                                      # the targets without in-edges


def test_restatement_follows_the_formula_edge_by_edge():
    """aggregate against the definition spelled out in Python floats: K = 2 kernels, D = 3 coordinates, M = 2 channels."""
    ei, n = graph_of("planted")
    g = torch.Generator().manual_seed(1)
    K, M, D = 2, 2, 3
    h, e = f32_exact((n, K * M), g), unit_coords((ei.size(1), D), g)
    mu, sigma = unit_coords((K, D), g), spread_sigma((K, D), g)
    for aggr in ("mean", "add"):
        want = torch.zeros(n, M, dtype=torch.float64)
        for i in range(n):
            into = [p for p in range(ei.size(1)) if int(ei[1, p]) == i]
            for p in into:
                for k in range(K):
                    q = sum(-0.5 * (float(e[p, d]) - float(mu[k, d])) ** 2 / (1e-15 + float(sigma[k, d]) ** 2)
                            for d in range(D))
                    want[i] += math.exp(q) * h[int(ei[0, p]), k * M:(k + 1) * M] / (len(into) if aggr == "mean" else 1)
        assert torch.allclose(aggregate(h, e, mu, sigma, n, ei[0], ei[1], aggr), want, rtol=0, atol=1e-12)


def test_restatement_sums_in_either_order():
    for graph in ("random", "planted"):
        case = operator_case(3, 5, 2, graph)
        a, b = run_formula(case, graph, "mean"), run_formula(case, graph, "mean", reverse=True)
        assert max(shares_of(b, a).values()) < 1e-6


def test_restatement_gradients_match_the_kernels_formulas():
    """The closed forms the edge pass evaluates, against autograd on the restatement:
    s = rs <h_j,k, gout_i> gauss; g_e = -sum_k s t, g_mu = sum_p s t, g_sigma = sum_p s t^2 sigma, t = (e - mu) / (eps + sigma^2)."""
    graph, (K, M, D) = "random", (3, 5, 2)
    case = operator_case(K, M, D, graph)
    ei, n = graph_of(graph)
    _, grads = reference(K, M, D, graph, "mean", True)
    h, e, mu, sigma, _, cot = case
    rs = 1.0 / torch.bincount(ei[1], minlength=n).clamp(min=1).double()
    E = ei.size(1)
    dots = (h[ei[0]].view(E, K, M) * cot[ei[1]].view(E, 1, M)).sum(-1)                 # [E, K]
    s = rs[ei[1]][:, None] * dots * gaussians(e, mu, sigma)
    t = (e.view(E, 1, D) - mu.view(1, K, D)) / (EPS + sigma.view(1, K, D) ** 2)
    assert torch.allclose(-(s[:, :, None] * t).sum(1), grads[1], rtol=0, atol=1e-10)
    assert torch.allclose((s[:, :, None] * t).sum(0), grads[2], rtol=0, atol=1e-10)
    assert torch.allclose((s[:, :, None] * t * t * sigma.view(1, K, D)).sum(0), grads[3], rtol=0, atol=1e-10)


def test_degree_pseudo_restated():
    """planted: in-degrees (2, 1, 3, 0, 0, 0); the edge 1 -> 0 gets (1 / sqrt(2), 1 / sqrt(3)), the self-loop 2 -> 2
    (1 / 2, 1 / 2), the edge 4 -> 2 (1, 1 / 2): a source without in-edges stays finite."""
    ei, n = graph_of("planted")
    u = degree_pseudo(ei, n)
    assert u.dtype == torch.float32 and u.shape == (6, 2) and bool(torch.isfinite(u).all())
    f = lambda v: torch.tensor(v, dtype=torch.float64).float()
    assert torch.equal(u[0], (1.0 / torch.sqrt(f([2.0, 3.0]))))
    assert u[5].tolist() == [0.5, 0.5] and u[3].tolist() == [1.0, 0.5]
    for name in ("random", "degrees"):
        ei, n = graph_of(name)
        u = degree_pseudo(ei, n)
        deg = torch.bincount(ei[1], minlength=n)
        assert float(u.min()) > 0 and float(u.max()) <= 1.0
        assert torch.allclose(u[:, 1].double() ** -2, (1 + deg[ei[1]]).double(), rtol=1e-6)


# ---- registry and module layout ----------------------------------------------------------------------------------------

def test_registry():
    from rgb_experiment_amd import nn as product_nn
    from rgb_experiment_amd.dist import experiment as dist_experiment
    from rgb_experiment_amd.models import MODELS, REGISTRY
    assert MODELS["monet"] is MoNet and "monet" not in REGISTRY
    assert "monet" not in dist_experiment.SUPPORTED
    assert "GMMConv" in product_nn.__all__ and product_nn.GMMConv is GMMConv
    assert list(inspect.signature(MoNet.__init__).parameters)[1:] == [
        "input_dim", "output_dim", "hidden_unit", "num_layers", "dropout_rate", "kernel_size", "dim"]
    assert inspect.signature(MoNet.__init__).parameters["dim"].default == 2
    assert list(inspect.signature(MoNet.forward).parameters)[1:] == ["x", "edge_index", "edge_attr"]
    assert inspect.signature(MoNet.forward).parameters["edge_attr"].default is None
    assert list(inspect.signature(GMMConv.__init__).parameters)[1:] == [
        "in_channels", "out_channels", "dim", "kernel_size", "separate_gaussians", "aggr", "root_weight", "bias"]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("root_weight", [True, False])
def test_parameter_names_shapes_and_strict_loading(root_weight, bias):
    conv = GMMConv(6, 7, 2, 3, root_weight=root_weight, bias=bias)
    want = {"g": (6, 21), "mu": (3, 2), "sigma": (3, 2)}
    if root_weight:
        want["root.weight"] = (7, 6)
    if bias:
        want["bias"] = (7,)
    assert {k: tuple(v.shape) for k, v in conv.named_parameters()} == want
    assert sorted(conv.state_dict()) == sorted(want)
    if bias:
        assert conv.bias.abs().max().item() == 0.0
    for name in ("g", "mu", "sigma"):                                     # glorot: U(-a, a), a = sqrt(6 / (rows + cols))
        p = getattr(conv, name)
        a = math.sqrt(6.0 / (p.size(0) + p.size(1)))
        assert 0.0 < p.abs().max().item() <= a
    if root_weight:
        assert 0.0 < conv.root.weight.abs().max().item() <= math.sqrt(6.0 / 13)
    ref = randomize(RefGMMConv(6, 7, 2, 3, root_weight=root_weight, bias=bias), 4)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    back = RefGMMConv(6, 7, 2, 3, root_weight=root_weight, bias=bias)
    back.load_state_dict({k: v.double() for k, v in conv.state_dict().items()}, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), ref.state_dict().values()))


def test_model_layout():
    x, y, ei, ea, model, ref = model_case()
    s = MODEL_SHAPE
    assert len(model.convs) == s["layers"] and all(isinstance(c, GMMConv) for c in model.convs)
    assert [(c.in_channels, c.out_channels, c.kernel_size, c.dim) for c in model.convs] == [
        (16, 12, 3, 2), (12, 12, 3, 2), (12, 5, 3, 2)]
    assert sorted(model.state_dict()) == sorted(ref.state_dict())
    back = copy.deepcopy(ref)
    back.load_state_dict({k: v.double() for k, v in model.state_dict().items()}, strict=True)
    for res in (ref(x, ei, ea), ref(x, ei)):
        assert set(res) == {"out", "emb"} and res["out"].shape == (s["n"], s["classes"])
    with pytest.raises(ValueError, match="num_layers"):
        MoNet(4, 3, 8, 0, 0.5, 2)


def test_kernel_channels_pads_what_the_layout_does_not_take():
    assert GMMConv(4, 67, 2, 3).kernel_channels() == 68
    assert GMMConv(4, 130, 2, 3).kernel_channels() == 132
    assert GMMConv(4, 64, 2, 3).kernel_channels() == 64 and GMMConv(4, 7, 2, 3).kernel_channels() == 7
    assert GMMConv(4, 256, 2, 3).kernel_channels() == 256


# ---- refusals ------------------------------------------------------------------------------------------------------

class HostCSR:
    def __init__(self, nnz, N):
        self.nnz, self.N = nnz, N


class HostGraph:
    def __init__(self, n, e, loops_mode=0):
        self.N, self.E, self.loops_mode = n, e, loops_mode
        self.fwd = HostCSR(e, n)


def test_layer_and_model_refusals():
    with pytest.raises(NotImplementedError, match="separate_gaussians"):
        GMMConv(4, 3, 2, 2, separate_gaussians=True)
    with pytest.raises(ValueError, match="in_channels"):
        GMMConv((4, 4), 3, 2, 2)
    for aggr in ("max", "min", "mul", None):
        with pytest.raises(ValueError, match="aggr"):
            GMMConv(4, 3, 2, 2, aggr=aggr)
    for aggr in ("mean", "add", "sum"):
        GMMConv(4, 3, 2, 2, aggr=aggr)
    with pytest.raises(ValueError, match="dim"):
        GMMConv(4, 3, 9, 2)
    with pytest.raises(ValueError, match="dim"):
        GMMConv(4, 3, 0, 2)
    with pytest.raises(ValueError, match="kernel_size"):
        GMMConv(4, 3, 2, 65)
    with pytest.raises(ValueError, match="kernel_size"):
        GMMConv(4, 3, 2, 0)
    with pytest.raises(ValueError, match="out_channels"):
        GMMConv(4, 257, 2, 2)
    GMMConv(4, 256, 8, 64)
    conv = GMMConv(4, 3, 2, 2)
    x, ei = torch.randn(5, 4), torch.tensor([[0, 1, 2], [1, 2, 3]])
    for bad in (None, torch.rand(3, 3), torch.rand(2, 2), torch.rand(3), torch.rand(3, 2).double(),
                torch.zeros(3, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="edge_attr"):
            conv(x, ei, bad)
    with pytest.raises(ValueError, match="in_channels"):
        conv(torch.randn(5, 3), ei, torch.rand(3, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(x, ei, torch.rand(3, 2))
    model = MoNet(4, 3, 8, 2, 0.0, 2, dim=3)
    with pytest.raises(ValueError, match="dim"):                          # degree coordinates are 2 wide
        model(x, ei)
    with pytest.raises(ValueError, match="edge_attr"):
        model(x, ei, torch.rand(3, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(x, ei, torch.rand(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MoNet(4, 3, 8, 2, 0.0, 2)(x, ei)


def test_operator_refusals():
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, LOOPS_REMOVE_ADD

    class Partitioned:
        is_distributed = True
    h, e, mu, sigma = torch.zeros(4, 8), torch.zeros(10, 2), torch.zeros(2, 2), torch.ones(2, 2)
    with pytest.raises(RuntimeError, match="no node-partitioned form"):
        ops.gmm_aggregate(h, e, mu, sigma, Partitioned())
    with pytest.raises(RuntimeError, match="no node-partitioned form"):
        ops.degree_pseudo(Partitioned())
    graph = HostGraph(4, 10)
    with pytest.raises(ValueError, match="aggr"):
        ops.gmm_aggregate(h, e, mu, sigma, graph, aggr="max")
    for mode in (LOOPS_ADD_REMAINING, LOOPS_REMOVE_ADD):
        with pytest.raises(RuntimeError, match="LOOPS_KEEP"):
            ops.gmm_aggregate(h, e, mu, sigma, HostGraph(4, 10, loops_mode=mode))
        with pytest.raises(RuntimeError, match="LOOPS_KEEP"):
            ops.degree_pseudo(HostGraph(4, 10, loops_mode=mode))
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.gmm_aggregate(torch.zeros(4, 7), e, mu, sigma, graph)          # 7 columns are no 2 blocks
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.gmm_aggregate(torch.zeros(3, 8), e, mu, sigma, graph)
    with pytest.raises(RuntimeError, match="e_slot"):
        ops.gmm_aggregate(h, torch.zeros(9, 2), mu, sigma, graph)
    with pytest.raises(RuntimeError, match="e_slot"):
        ops.gmm_aggregate(h, torch.zeros(10, 3), mu, sigma, graph)
    with pytest.raises(RuntimeError, match="mu and sigma"):
        ops.gmm_aggregate(h, e, mu, torch.ones(2, 3), graph)
    with pytest.raises(RuntimeError, match="y0"):
        ops.gmm_aggregate(h, e, mu, sigma, graph, y0=torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gmm_aggregate(h, e, mu, sigma, graph)


# ---- experiment(model_name="monet") ---------------------------------------------------------------------------------------

MONET_INIT = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0, "kernel_size": 3, "dim": 2}


def test_experiment_plumbing():
    run = G._run
    attr = torch.rand(300, 2, generator=torch.Generator().manual_seed(7))
    monet = dict(model_name="monet", init=MONET_INIT)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # degree coordinates: the device check is next
        run(G._data(False), **monet)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # an unused data.edge_attr changes nothing
        run(G._data(True), **monet)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        run(G._data(True, attr), use_edge_attr=True, **monet)
    # a wrong data.edge_attr is refused before that
    with pytest.raises(ValueError, match="needs data.edge_attr"):
        run(G._data(False), use_edge_attr=True, **monet)
    with pytest.raises(ValueError, match="needs data.edge_attr"):
        run(G._data(True, torch.zeros(300, 2, dtype=torch.int64)), use_edge_attr=True, **monet)
    with pytest.raises(ValueError, match=r"\[E, D\]"):
        run(G._data(True, torch.zeros(299, 2)), use_edge_attr=True, **monet)
    with pytest.raises(ValueError, match="to_undirected"):
        run(G._data(True, attr), use_edge_attr=True, to_undirected_graph=True, **monet)
    with pytest.raises(NotImplementedError, match="partitioned"):
        run(G._data(True, attr), use_edge_attr=True, distributed=True, **monet)
    # (a width other than the model's dim, and dim != 2 without attributes, are the layer's and the model's refusals:
    # test_layer_and_model_refusals)
    # the other edge flags keep their refusals
    with pytest.raises(ValueError, match="takes no edge attributes"):
        run(G._data(True), model_name="gcn", use_edge_attr=True)
    with pytest.raises(ValueError, match="takes no edge types"):
        run(G._data(True), use_edge_type=True, **monet)
    with pytest.raises(ValueError, match="takes no edge weights"):
        run(G._data(True), use_edge_weight=True, **monet)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

NEW_ENTRIES = ("rgbx_gmm_supported", "rgbx_gmm_fwd_f32", "rgbx_gmm_bwd_src_f32", "rgbx_gmm_bwd_edge_workspace_bytes",
               "rgbx_gmm_bwd_edge_f32", "rgbx_gmm_degree_pseudo_f32")


def loaded_lib():
    from rgb_experiment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_abi_declares_and_exports_the_new_entries():
    from rgb_experiment_amd import _lib
    raw = open(os.path.join(ROOT, "include", "rgbx_hip.h")).read()
    assert "GMMConv.message [PyG]" in raw and "gaussian.sum(dim=-1)" in raw   # the PyG lines the family replaces
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(rgbx_[a-z0-9_]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS, name
        params = re.search(name + r"\s*\(([^)]*)\)", text).group(1)       # one ctypes argument per declared parameter
        assert len(_lib.SIGNATURES[name]) == len([a for a in params.split(",") if a.strip()]), name
    assert loaded_lib().rgbx_version() == 501


def test_supported_over_the_gpu_grid():
    lib = loaded_lib()
    for K, M in PAIRS:
        for D in DIMS:
            assert lib.rgbx_gmm_supported(K, M, D), (K, M, D)
    for M in range(1, 301):                                               # the widths of the shared lane layout
        assert bool(lib.rgbx_gmm_supported(2, M, 2)) == bool(lib.rgbx_transformer_supported(2, M)), M
    assert not lib.rgbx_gmm_supported(2, PADDED_WIDTH, 2) and lib.rgbx_gmm_supported(2, PADDED_WIDTH + 1, 2)
    assert lib.rgbx_gmm_supported(64, 8, 8) and not lib.rgbx_gmm_supported(65, 8, 8)
    assert not lib.rgbx_gmm_supported(0, 8, 2) and not lib.rgbx_gmm_supported(2, 0, 2)
    assert not lib.rgbx_gmm_supported(2, 8, 0) and not lib.rgbx_gmm_supported(2, 8, 9) and lib.rgbx_gmm_supported(2, 8, 1)
    vec = lambda M: 4 if M % 4 == 0 else (2 if M % 2 == 0 else 1)
    assert {vec(M) for _, M in PAIRS} == {1, 2, 4} and {vec(M) for _, M in SWEEP_PAIRS} == {1, 2, 4}
    pow2ceil = lambda v: 1 << (v - 1).bit_length()
    chunks = lambda K, M: -(-K // min(K, 64 // pow2ceil(-(-M // vec(M)))))
    assert chunks(2, 66) > 1 and chunks(8, 40) > 1                         # heads in several chunks
    assert chunks(3, 5) == 1 and chunks(8, 16) == 1 and chunks(4, 64) == 1 and chunks(1, 256) == 1   # and in one


def workspace_bytes(lib, nnz, K, D):
    n = ctypes.c_size_t(0)
    assert lib.rgbx_gmm_bwd_edge_workspace_bytes(nnz, K, D, ctypes.byref(n)) == 0
    return n.value


def test_new_entries_validate_their_arguments():
    lib = loaded_lib()
    p = 0x10000  # 16-byte aligned, non-null, never dereferenced: every call below returns before a launch
    q = p + 0x100000

    def fwd(**kw):
        a = dict(rowptr=p, col=p, e=p, lde=2, mu=p, sigma=p, rs=p, h=p, ldh=128, y0=p, ldy=64, out=q, ldo=64, N=10, K=2,
                 M=64, D=2)
        a.update(kw)
        return lib.rgbx_gmm_fwd_f32(a["rowptr"], a["col"], a["e"], a["lde"], a["mu"], a["sigma"], a["rs"], a["h"], a["ldh"],
                                    a["y0"], a["ldy"], a["out"], a["ldo"], a["N"], a["K"], a["M"], a["D"], None, None)
    for name in ("rowptr", "col", "e", "mu", "sigma", "h", "out"):
        assert fwd(**{name: None}) == -1 and b"null" in lib.rgbx_last_error_string(), name
    assert fwd(ldh=127) == -1 and b"leading dimension" in lib.rgbx_last_error_string()
    assert fwd(ldo=63) == -1 and fwd(ldy=8) == -1 and fwd(lde=1) == -1
    assert fwd(out=p) == -1 and b"alias" in lib.rgbx_last_error_string()
    assert fwd(N=-1) == -1 and fwd(K=0) == -1 and fwd(M=0) == -1
    assert fwd(N=2 ** 31) == -2                                            # RGBX_E_RANGE
    assert fwd(D=0) == -5 and fwd(D=9, lde=9) == -5 and fwd(K=65, ldh=65 * 64) == -5   # RGBX_E_SHAPE
    assert fwd(M=67, ldh=134, ldy=67, ldo=67) == -5
    assert fwd(h=p + 2) == -3 and b"aligned" in lib.rgbx_last_error_string()
    assert fwd(e=p + 1) == -3 and fwd(mu=p + 2) == -3 and fwd(sigma=p + 3) == -3 and fwd(rs=p + 2) == -3
    assert fwd(y0=p + 2) == -3
    # M = 256 needs 4 floats per lane: 16-byte pointers and leading dimensions that are multiples of 4
    wide = dict(M=256, ldh=512, ldy=256, ldo=256)
    assert fwd(**{**wide, "h": p + 8}) == -5 and b"lanes" in lib.rgbx_last_error_string()
    assert fwd(**{**wide, "ldh": 514}) == -5
    assert fwd(N=0) == 0 and fwd(N=0, rowptr=None) == 0

    def src(**kw):
        a = dict(t2f=p, w_t=p, e=p, lde=2, mu=p, sigma=p, gout=p, ldg=64, g_h=q, ldgh=128, N=1000, K=2, M=64, D=2)
        a.update(kw)
        return lib.rgbx_gmm_bwd_src_f32(p, p, a["t2f"], a["w_t"], a["e"], a["lde"], a["mu"], a["sigma"], a["gout"], a["ldg"],
                                        a["g_h"], a["ldgh"], a["N"], a["K"], a["M"], a["D"], None, None)
    for name in ("t2f", "e", "mu", "sigma", "gout", "g_h"):
        assert src(**{name: None}) == -1, name
    assert src(ldg=63) == -1 and src(ldgh=127) == -1 and src(lde=1) == -1 and src(g_h=p) == -1
    assert src(K=-1) == -1 and src(D=0) == -5 and src(D=9, lde=9) == -5 and src(K=65, ldgh=65 * 64) == -5
    assert src(gout=p + 2) == -3 and src(g_h=q + 1) == -3 and src(mu=p + 2) == -3 and src(w_t=p + 1) == -3
    assert src(M=130, ldg=130, ldgh=260) == -5
    assert src(N=2 ** 31) == -2 and src(N=0) == 0

    need = workspace_bytes(lib, 5000, 2, 2)
    assert need >= 4 * 5000 * 2 and need % 4 == 0
    assert workspace_bytes(lib, 0, 2, 2) == 0 and workspace_bytes(lib, 5000, 8, 8) > workspace_bytes(lib, 5000, 8, 1)
    n = ctypes.c_size_t(0)
    assert lib.rgbx_gmm_bwd_edge_workspace_bytes(5000, 2, 2, None) == -1
    assert lib.rgbx_gmm_bwd_edge_workspace_bytes(-1, 2, 2, ctypes.byref(n)) == -1
    assert lib.rgbx_gmm_bwd_edge_workspace_bytes(2 ** 31, 2, 2, ctypes.byref(n)) == -2

    def edge(**kw):
        a = dict(rowptr=p, col=p, e=p, lde=2, mu=p, sigma=p, rs=p, h=p, ldh=128, gout=p, ldg=64, g_e=q, ldge=2,
                 g_mu=q + 0x100000, g_sigma=q + 0x200000, ws=q + 0x300000, ws_bytes=need, N=1000, nnz=5000, K=2, M=64, D=2)
        a.update(kw)
        return lib.rgbx_gmm_bwd_edge_f32(a["rowptr"], a["col"], a["e"], a["lde"], a["mu"], a["sigma"], a["rs"], a["h"],
                                         a["ldh"], a["gout"], a["ldg"], a["g_e"], a["ldge"], a["g_mu"], a["g_sigma"],
                                         a["ws"], a["ws_bytes"], a["N"], a["nnz"], a["K"], a["M"], a["D"], None, None)
    for name in ("rowptr", "col", "e", "mu", "sigma", "h", "gout"):
        assert edge(**{name: None}) == -1 and b"null" in lib.rgbx_last_error_string(), name
    assert edge(g_mu=None) == -1 and edge(g_sigma=None) == -1 and b"both or neither" in lib.rgbx_last_error_string()
    assert edge(g_e=None, g_mu=None, g_sigma=None) == 0                   # nothing asked for, nothing launched
    assert edge(ldh=127) == -1 and edge(ldg=63) == -1 and edge(lde=1) == -1 and edge(ldge=1) == -1
    assert edge(g_e=p) == -1 and b"alias" in lib.rgbx_last_error_string()
    assert edge(nnz=-1) == -1 and edge(nnz=2 ** 31) == -2 and edge(N=2 ** 31) == -2
    assert edge(D=0) == -5 and edge(D=9, lde=9, ldge=9) == -5 and edge(K=65, ldh=65 * 64) == -5 and edge(M=67) == -5
    assert edge(h=p + 2) == -3 and edge(g_e=q + 2) == -3 and edge(g_mu=q + 0x100001) == -3 and edge(ws=q + 0x300002) == -3
    assert edge(ws_bytes=need - 4) == -4 and b"workspace" in lib.rgbx_last_error_string()
    assert edge(ws=None) == -4 and edge(ws_bytes=0) == -4
    assert edge(g_mu=None, g_sigma=None, ws_bytes=need - 4) == -4         # the table s is needed for g_e alone too

    def pseudo(**kw):
        a = dict(rowptr=p, col=p, u=q, N=10)
        a.update(kw)
        return lib.rgbx_gmm_degree_pseudo_f32(a["rowptr"], a["col"], a["u"], a["N"], None, None)
    for name in ("rowptr", "col", "u"):
        assert pseudo(**{name: None}) == -1 and b"null" in lib.rgbx_last_error_string(), name
    assert pseudo(N=-1) == -1 and pseudo(N=2 ** 31) == -2 and pseudo(u=q + 2) == -3 and pseudo(col=p + 1) == -3
    assert pseudo(N=0) == 0 and pseudo(N=0, rowptr=None) == 0


# ---- preconditions of the GPU cases ----------------------------------------------------------------------------------

def test_cases_cover_what_the_issue_lists():
    from rgb_experiment_amd.graph import LONG_ROW_SLOTS as product_threshold
    assert LONG_ROW_SLOTS == product_threshold
    assert {(K, M) for K, M, *_ in CASES} == set(PAIRS) and {D for _, _, D, *_ in CASES} == set(DIMS)
    for K, M in SWEEP_PAIRS:
        assert {g for k, m, _, g, _, _ in CASES if (k, m) == (K, M)} >= set(graph_names)
    assert {a for *_, a, _ in CASES} == {"mean", "sum", "add"} and {y for *_, y in CASES} == {True, False}
    for K, M, D, graph, _, _ in CASES:                                    # the inputs are where the docstring says
        h, e, mu, sigma, y0, cot = operator_case(K, M, D, graph)
        assert e.numel() == 0 or (float(e.min()) >= 0.0 and float(e.max()) < 1.0)
        assert float(mu.min()) >= 0.0 and float(mu.max()) < 1.0
        assert 0.5 <= float(sigma.abs().min()) and float(sigma.abs().max()) < 1.5
        assert all(torch.equal(t.float().double(), t) for t in (h, e, mu, sigma, y0, cot))
    signs = torch.cat([operator_case(K, M, D, g)[3].flatten() for K, M, D, g, _, _ in CASES])
    assert bool((signs < 0).any()) and bool((signs > 0).any())
    assert float(gaussians(*operator_case(8, 16, 8, "powerlaw")[1:4]).min()) > math.exp(-16.0)   # no Gaussian underflows


@pytest.mark.parametrize("K,M,D,graph,aggr,with_y0", CASES)
def test_operator_case_is_well_posed(K, M, D, graph, aggr, with_y0):
    aggr = "add" if aggr == "sum" else aggr
    want = reference(K, M, D, graph, aggr, with_y0)
    got = run_formula(operator_case(K, M, D, graph), graph, aggr, with_y0, dtype=torch.float32, reverse=True)
    shares = shares_of(got, want)
    assert max(shares.values()) < WELL_POSED_SHARE, shares
    if graph == "no_edges":
        assert torch.equal(want[0], operator_case(K, M, D, graph)[4])      # out == y0
        assert all(float(t.abs().max()) == 0.0 for t in want[1][:1] + want[1][2:4]) and want[1][1].shape == (0, D)


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
    x, ei, ea, ref = layer_case(name)
    shares = module_shares(ref, lambda m, dt, rev: m(x.to(dt), ei, ea.to(dt), rev), 17)
    assert max(shares.values()) < WELL_POSED_SHARE, shares


@pytest.mark.parametrize("with_attr", [True, False])
def test_model_case_is_well_posed(with_attr):
    x, y, ei, ea, model, ref = model_case()
    ref.train()
    shares = module_shares(ref, lambda m, dt, rev: m(x.to(dt), ei, ea.to(dt) if with_attr else None, rev)["out"], 18)
    assert max(shares.values()) < WELL_POSED_SHARE, shares


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_case_is_supported_and_well_posed(seed):
    K, M, D, aggr, with_y0, ei, n, case = fuzz_case(seed)
    assert loaded_lib().rgbx_gmm_supported(K, M, D), (K, M, D)
    shares = shares_of(run_fuzz(seed, torch.float32, True), run_fuzz(seed))
    assert max(shares.values()) < WELL_POSED_SHARE, shares


def test_fuzz_seeds_spread_over_the_dispatch_space():
    drawn = [fuzz_case(seed)[:5] + (fuzz_case(seed)[5].size(1),) for seed in FUZZ_SEEDS]
    vec = lambda M: 4 if M % 4 == 0 else (2 if M % 2 == 0 else 1)
    assert {vec(M) for _, M, *_ in drawn} == {1, 2, 4}
    assert len({D for _, _, D, *_ in drawn}) >= 6 and {a for _, _, _, a, _, _ in drawn} == {"mean", "sum"}
    assert {y for *_, y, _ in drawn} == {True, False}
    assert max(E for *_, E in drawn) > LONG_ROW_SLOTS and min(K for K, *_ in drawn) == 1 and max(K for K, *_ in drawn) >= 8
