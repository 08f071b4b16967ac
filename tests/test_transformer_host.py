"""TransformerConv on the host: a float64 restatement of the layer (scaled dot-product attention over the in-edges AS
GIVEN, root skip, beta gate) pinned by numbers derived by hand and by torch's scaled_dot_product_attention under the
adjacency mask; registry, module layout (PyG's names, strict state_dict loading), refusals and the C ABI of the new entry
points; and the case builders tests/test_gpu_transformer.py feeds to the HIP kernels, with the checks that keep those
cases well-posed. No GPU needed.

Well-posedness. Every operator, layer, model and large-score case is run through the restatement in float32 on the CPU
and has to stay within a QUARTER of the GPU test's tolerances (forward 1e-4, gradients 2e-4, times max(1, |ref|max))
of the float64 result: a condition on the inputs, not on a kernel.

Large scores. q and k of the order-1 operator case are multiplied by LARGE_Q_SCALE and LARGE_K_SCALE (powers of two:
the values stay exactly representable in float32), v and the cotangent stay where they were; on `powerlaw` a few key
rows are then replaced so that long rows get their maximum late in the CSR slot order and the hub row's chunks get
maxima far apart. Reached range (printed by test_large_case_is_in_range_and_well_posed): scores of standard deviation
128; |e| up to 876 at (8, 8) and 642 at (1, 64) on `random`, up to 1654 and 624 on `powerlaw` (the planted maxima and
what they do to the other rows of their sources), far above log FLT_MAX = 88.7; the float32 restatement uses up to 0.18
of the tolerance ((8, 8) on `powerlaw`, forward). The scales are the largest powers of two the quarter share permits:
at the next one (standard deviation 256) the same case uses 0.35, as a score of a thousand rounds at ulp(e) = 6e-5 and
every softmax weight inherits that."""
import copy
import ctypes
import functools
import itertools
import math
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FWD_TOL, GRAD_TOL = 1e-4, 2e-4          # the project's tolerances (tests/test_gpu_gatv2.py), used unchanged on the GPU
WELL_POSED_SHARE = 0.25                 # float32-vs-float64 on the CPU may use this share of them
LONG_ROW_SLOTS = 1024                   # rgb_experiment_amd.graph.LONG_ROW_SLOTS (asserted below)


# ---- the restatement ---------------------------------------------------------------------------------------------------

def attend(q, k, v, n, src, dst, scale, keep=None, p=0.0):
    """out [n, H, C] and the scores e [E, H] from q, k, v [n, H, C], in the precision of the inputs. The edges are taken
    as given; `keep` bool [E, H] (True = kept) are the dropout decisions; a node without in-edges gets zeros."""
    H, C = q.size(1), q.size(2)
    e = (q[dst] * k[src]).sum(-1) * scale                                           # [E, H]
    idx = dst.view(-1, 1).expand(-1, H)
    mx = torch.full((n, H), -1e30, dtype=e.dtype).scatter_reduce(0, idx, e.detach(), "amax")
    ex = torch.exp(e - mx[dst])
    den = torch.zeros(n, H, dtype=e.dtype).index_add(0, dst, ex)
    alpha = ex / (den[dst] + 1e-16)
    if keep is not None:
        alpha = alpha * keep.to(e.dtype) / (1.0 - p)
    return torch.zeros(n, H, C, dtype=e.dtype).index_add(0, dst, alpha.unsqueeze(-1) * v[src]), e


class RefTransformerConv(nn.Module):
    """float64 restatement of TransformerConv, written from the formulas of the layer's contract; PyG's parameter names
    (the three projections always carry a bias, `bias` is lin_skip's; lin_skip exists without root_weight too, unused).
    The dropout decisions are INPUTS (`choices`): 'src' / 'dst' (the edges in the order the mask refers to) and 'keep'
    bool [E, H]. Without `choices` the edges are edge_index's and nothing is dropped."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, bias=True,
                 root_weight=True):
        super().__init__()
        self.H, self.C, self.concat, self.p, self.root_weight = heads, out_channels, concat, dropout, root_weight
        wide = heads * out_channels
        self.lin_key = nn.Linear(in_channels, wide).double()
        self.lin_query = nn.Linear(in_channels, wide).double()
        self.lin_value = nn.Linear(in_channels, wide).double()
        self.lin_skip = nn.Linear(in_channels, wide if concat else out_channels, bias=bias).double()
        self.lin_beta = (nn.Linear(3 * (wide if concat else out_channels), 1, bias=False).double()
                         if beta and root_weight else None)

    def forward(self, x, ei, choices=None):
        n, H, C = x.size(0), self.H, self.C
        src, dst = (ei[0], ei[1]) if choices is None else (choices["src"], choices["dst"])
        keep = choices["keep"] if (choices is not None and self.training and self.p > 0) else None
        out, e = attend(self.lin_query(x).view(n, H, C), self.lin_key(x).view(n, H, C), self.lin_value(x).view(n, H, C),
                        n, src, dst, 1.0 / math.sqrt(C), keep, self.p)
        self.e = e.detach()
        out = out.reshape(n, H * C) if self.concat else out.mean(1)
        if self.root_weight:
            x_r = self.lin_skip(x)
            if self.lin_beta is not None:
                b = torch.sigmoid(self.lin_beta(torch.cat([out, x_r, out - x_r], dim=-1)))
                out = b * x_r + (1.0 - b) * out
            else:
                out = out + x_r
        return out


class RefGraphTransformer(nn.Module):
    """models/transformer.py in float64: (TransformerConv -> BatchNorm1d) x (L - 1), TransformerConv(hid * heads, out, 1,
    concat=False); the product's module names. `choices`: one entry per layer (None = nothing dropped)."""

    def __init__(self, num_layers, hidden_unit, input_dim, output_dim, heads, att_dropout=0.0, beta=False,
                 root_weight=True):
        super().__init__()
        wide = hidden_unit * heads
        kw = dict(dropout=att_dropout, beta=beta, root_weight=root_weight)
        self.convs = nn.ModuleList(
            [RefTransformerConv(input_dim if i == 0 else wide, hidden_unit, heads, **kw) for i in range(num_layers - 1)]
            + [RefTransformerConv(wide, output_dim, 1, concat=False, **kw)])
        self.bns = nn.ModuleList(nn.BatchNorm1d(wide).double() for _ in range(num_layers - 1))

    def forward(self, x, ei, choices=None):
        choices = [None] * len(self.convs) if choices is None else choices
        for i, conv in enumerate(self.convs):
            x = conv(x, ei, choices[i])
            if i < len(self.bns):
                x = self.bns[i](x)
        return {"out": F.log_softmax(x, dim=1), "emb": x}


# ---- graphs and cases shared with tests/test_gpu_transformer.py -----------------------------------------------------------

PAIRS = [(1, 4), (1, 7), (2, 8), (8, 8), (3, 5), (8, 40), (1, 64), (1, 256)]  # (8, 40): heads in several chunks
GRAPH_NAMES = ("no_edges", "powerlaw", "random")


@functools.lru_cache(maxsize=None)
def graph_of(name):
    """(edge_index, n), built once. `random`: every edge INTO nodes 0 .. 19 and every edge OUT OF nodes 20 .. 39 removed, so
    that rows without in-edges and sources without out-edges exist in numbers."""
    from test_gpu_fagcn import powerlaw_graph
    from test_gpu_ggnn import rand_graph
    if name == "no_edges":
        return torch.zeros((2, 0), dtype=torch.int64), 50
    if name == "random":
        ei = rand_graph(700, 6000, 3, loops=11, dups=40)
        return ei[:, (ei[1] >= 20) & ~((ei[0] >= 20) & (ei[0] < 40))].contiguous(), 700
    if name == "powerlaw":
        return powerlaw_graph(), 2000
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def slots_of(name):
    """(src, dst) of the edges as given, the CSR's (rowptr, order): slot p of the target-grouped CSR is edge order[p] (a
    stable grouping by target, which the device's CSR build is: tests/test_gpu_parity.py::test_csr_build_bit_exact)."""
    ei, n = graph_of(name)
    order = torch.argsort(ei[1], stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(ei[1], minlength=n), 0)
    return ei[0], ei[1], rowptr, order


def f32_exact(shape, gen, scale=1.0):
    """float64 values that are exactly representable in float32: both sides of a comparison hold the same numbers."""
    return (torch.randn(shape, generator=gen) * scale).double()


@functools.lru_cache(maxsize=None)
def operator_case(H, C, graph_name):
    """q, k, v [n, H*C] ~ N(0, 1) (scores <q, k> / sqrt(C) of order 1) and the cotangent: float64, fp32-exact."""
    _, n = graph_of(graph_name)
    g = torch.Generator().manual_seed(2000 + 10 * H + C)
    return tuple(f32_exact((n, H * C), g) for _ in range(4))


def run_formula(case, graph_name, H, C, dtype=torch.float64, src=None, dst=None, keep=None, p=0.0):
    """The restatement's attention on a case in `dtype`: (out [n, H*C], [g_q, g_k, g_v], e)."""
    _, n = graph_of(graph_name)
    if src is None:
        src, dst, _, _ = slots_of(graph_name)
    q, k, v = (t.to(dtype).clone().requires_grad_(True) for t in case[:3])
    out, e = attend(q.view(n, H, C), k.view(n, H, C), v.view(n, H, C), n, src, dst, 1.0 / math.sqrt(C), keep, p)
    out = out.reshape(n, H * C)
    (out * case[3].to(dtype)).sum().backward()
    return out.detach(), [q.grad, k.grad, v.grad], e.detach()


@functools.lru_cache(maxsize=None)
def eval_reference(H, C, graph_name, large=False):
    return run_formula(large_case(H, C, graph_name) if large else operator_case(H, C, graph_name), graph_name, H, C)


def share_of_tolerance(got, want, tol):
    """max |got - want| as a share of tol * max(1, |want|max): `close` passes below 1."""
    return (got.detach().double() - want.detach()).abs().max().item() / (tol * max(1.0, want.detach().abs().max().item()))


NAMES = ("forward", "g_q", "g_k", "g_v")


def shares_of(got, want):
    out = {"forward": share_of_tolerance(got[0], want[0], FWD_TOL)}
    for name, a, b in zip(NAMES[1:], got[1], want[1]):
        out[name] = share_of_tolerance(a, b, GRAD_TOL)
    return out


# ---- large scores ---------------------------------------------------------------------------------------------------------

LARGE_PAIRS = [(8, 8), (1, 64)]
LARGE_GRAPHS = ("random", "powerlaw")
LARGE_Q_SCALE, LARGE_K_SCALE = 16.0, 8.0  # scores of standard deviation 128
SPIKE_ABOVE = 60.0                        # a planted maximum sits this far above every unplanted score
SPIKE_ROWS = 40                           # the longest rows of `powerlaw` get one


@functools.lru_cache(maxsize=None)
def large_case(H, C, graph_name):
    """operator_case with q and k scaled (powers of two: still fp32-exact). On `powerlaw`, for each of the SPIKE_ROWS longest
    rows r and one head h = r % H, the key row of a source j that occurs only in the LAST quarter of r's slots is replaced
    by a multiple of q[r, h] such that e(r, j) = max |e| + SPIKE_ABOVE: the row's maximum arrives after the accumulator
    has filled. The hub row (above LONG_ROW_SLOTS, cut into chunks) gets, for H >= 2, a second head whose maximum sits in
    its FIRST chunk: chunk states with maxima far apart, in both orders, meet in one combine."""
    q, k, v, cot = operator_case(H, C, graph_name)
    q, k = q * LARGE_Q_SCALE, (k * LARGE_K_SCALE).clone()
    if graph_name != "powerlaw":
        return q, k, v, cot
    _, n = graph_of(graph_name)
    src, dst, rowptr, order = slots_of(graph_name)
    scale = 1.0 / math.sqrt(C)
    top = ((q.view(n, H, C)[dst] * k.view(n, H, C)[src]).sum(-1) * scale).abs().max().item() + SPIKE_ABOVE
    deg = rowptr[1:] - rowptr[:-1]
    used = set()

    def plant(r, h, lo, hi):
        """Head h of a source seen in slots [lo, hi) of row r and nowhere else in the row: e(r, that source) = top."""
        slots = src[order[rowptr[r]:rowptr[r + 1]]]
        inside = set(slots[lo:hi].tolist())
        outside = set(slots[:lo].tolist()) | set(slots[hi:].tolist())
        for j in slots[lo:hi].tolist():
            if j in outside or j in used or j == r:
                continue
            qr = q[r, h * C:(h + 1) * C]
            k[j, h * C:(h + 1) * C] = (qr * (top / scale / (qr * qr).sum())).float().double()
            used.add(j)
            return True
        return False
    for r in torch.argsort(deg, descending=True, stable=True)[:SPIKE_ROWS].tolist():
        d = int(deg[r])
        plant(r, r % H, d - d // 4, d)
        if d > LONG_ROW_SLOTS and H >= 2:
            plant(r, (r + 1) % H, 0, LONG_ROW_SLOTS // 2)
    return q, k, v, cot


def score_profile(e, graph_name):
    """`e` [E, H] in edge order -> {'max_abs', 'late_rows': rows of >= 65 slots with a head whose maximum sits in the last
    quarter of the slot order and >= 40 above everything before it, 'chunks': where ('first' / 'last' / 'middle') the
    maximum of a head of a hub row sits when its chunk maxima are >= 40 apart}."""
    _, _, rowptr, order = slots_of(graph_name)
    es = e[order]
    H = e.size(1)
    deg = rowptr[1:] - rowptr[:-1]
    late_rows, chunk_hits = 0, set()
    for r in torch.nonzero(deg >= 65).view(-1).tolist():
        row = es[rowptr[r]:rowptr[r + 1]]
        d = row.size(0)
        at = row.argmax(0)
        before = torch.cat([torch.full((1, H), -1e30, dtype=row.dtype), torch.cummax(row, 0)[0]])[at, torch.arange(H)]
        late_rows += int(((at >= 0.75 * d) & (row.max(0)[0] - before >= 40)).any())
        if d > LONG_ROW_SLOTS:
            cmax = torch.stack([c.max(0)[0] for c in row.split(LONG_ROW_SLOTS)])
            last = (d - 1) // LONG_ROW_SLOTS
            for h in range(H):
                if cmax[:, h].max() - cmax[:, h].min() >= 40:
                    c = int(at[h]) // LONG_ROW_SLOTS
                    chunk_hits.add("first" if c == 0 else "last" if c == last else "middle")
    return {"max_abs": e.abs().max().item(), "late_rows": late_rows, "chunks": chunk_hits}


# ---- layer and model cases ------------------------------------------------------------------------------------------------

LAYER_N, LAYER_E, LAYER_F = 120, 500, 12
LAYER_CASES = {  # name -> (H, C, layer keywords)
    "default": (2, 8, dict()),
    "mean_of_3_heads": (3, 5, dict(concat=False)),
    "beta": (2, 8, dict(beta=True)),
    "beta_mean": (3, 5, dict(beta=True, concat=False)),
    "no_root": (2, 8, dict(root_weight=False)),
    "no_bias": (2, 8, dict(bias=False)),
    "padded_67": (2, 67, dict()),
    "padded_130": (1, 130, dict()),
}


def layer_case(name, p=0.0):
    """(x float64 fp32-exact, edge_index, reference layer with every parameter set to fp32-exact random values)."""
    from test_gpu_ggnn import rand_graph
    H, C, kw = LAYER_CASES[name]
    g = torch.Generator().manual_seed(7100)
    ei = rand_graph(LAYER_N, LAYER_E, 7100, loops=5, dups=12)
    x = f32_exact((LAYER_N, LAYER_F), g)
    ref = RefTransformerConv(LAYER_F, C, heads=H, dropout=p, **kw)
    with torch.no_grad():
        for key, prm in ref.named_parameters():
            prm.copy_(f32_exact(prm.shape, g, prm.size(-1) ** -0.5 if key.endswith("weight") else 0.5))
    return x, ei, ref


MODEL_SHAPE = dict(n=60, e=240, f=16, hidden=4, heads=2, classes=5, layers=3)


def model_case(**kw):
    """(x, y, edge_index, the product's model on the CPU, the reference holding the same parameters)."""
    from rgb_experiment_amd.models import GraphTransformer
    from test_gpu_ggnn import rand_graph
    s = MODEL_SHAPE
    g = torch.Generator().manual_seed(9100)
    ei = rand_graph(s["n"], s["e"], 9100, loops=3, dups=6)
    x = f32_exact((s["n"], s["f"]), g)
    y = torch.randint(0, s["classes"], (s["n"],), generator=g)
    torch.manual_seed(9100)
    model = GraphTransformer(s["layers"], s["hidden"], s["f"], s["classes"], 0.0, s["heads"], **kw)
    with torch.no_grad():  # biases off zero, so that their paths are exercised
        for key, prm in model.named_parameters():
            if key.endswith("bias"):
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.3)
    ref = RefGraphTransformer(s["layers"], s["hidden"], s["f"], s["classes"], s["heads"], **kw)
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()},
                        strict=True)
    return x, y, ei, model, ref


def synthetic_keep(n_edges, H, seed):
    """Dropout decisions at p = 0.5 for the host-side checks (the GPU test feeds the device's own)."""
    return torch.rand((n_edges, H), generator=torch.Generator().manual_seed(seed)) >= 0.5


# ---- the restatement is pinned ---------------------------------------------------------------------------------------------

def test_restatement_reproduces_hand_computed_numbers():
    """4 nodes, one head of two channels, 5 edges: 0 -> 1 twice (a duplicate), 2 -> 1, 1 -> 1 (a self-loop), 3 -> 2; nodes
    0 and 3 have no in-edge. q_i = sqrt(2) a_i and scale = 1 / sqrt(2), so e = <a_i, k_j>. Derived edge by edge with scalar
    arithmetic from the contract's formulas, not with the code under test:
      target 1 (a = (0, 1)): e = 0, 0 (k_0 = (1, 0), counted twice), 1 (k_2 = (1, 1)), 2 (k_1 = (0, 2));
        weights 1, 1, E, E^2 over s = 2 + E + E^2;
        out_1 = (2 v_0 + E v_2 + E^2 v_1) / s = ((2 + 2E) / s, (2E + E^2) / s)   with v_0 = (1, 0), v_2 = (2, 2), v_1 = (0, 1)
      target 2 (a = (1, 1)): one edge, e = <(1, 1), (-1, 0)> = -1, weight 1, out_2 = v_3 = (-1, 3)
      targets 0 and 3: no in-edge, zeros."""
    r2 = math.sqrt(2.0)
    t = lambda rows: torch.tensor(rows, dtype=torch.float64)
    q = t([[1, 0], [0, 1], [1, 1], [1, -1]]) * r2
    k = t([[1, 0], [0, 2], [1, 1], [-1, 0]])
    v = t([[1, 0], [0, 1], [2, 2], [-1, 3]])
    src, dst = torch.tensor([0, 0, 2, 1, 3]), torch.tensor([1, 1, 1, 1, 2])
    out, e = attend(q.view(4, 1, 2), k.view(4, 1, 2), v.view(4, 1, 2), 4, src, dst, 1.0 / r2)
    E = math.e
    s = 2 + E + E * E
    assert torch.allclose(e[:, 0], t([0, 0, 1, 2, -1]), rtol=0, atol=1e-12)
    want = t([[0, 0], [(2 + 2 * E) / s, (2 * E + E * E) / s], [-1, 3], [0, 0]])
    assert torch.allclose(out[:, 0], want, rtol=0, atol=1e-12)
    assert out[0].abs().max().item() == 0.0 and out[3].abs().max().item() == 0.0
    # dropout at p = 0.5 with slot 2 (2 -> 1) dropped: out_1 = 2 (2 v_0 + E^2 v_1) / s; the normaliser is the undropped one
    keep = torch.tensor([[1], [1], [0], [1], [1]], dtype=torch.bool)
    out_d, _ = attend(q.view(4, 1, 2), k.view(4, 1, 2), v.view(4, 1, 2), 4, src, dst, 1.0 / r2, keep, 0.5)
    assert torch.allclose(out_d[:, 0], t([[0, 0], [4 / s, 2 * E * E / s], [-2, 6], [0, 0]]), rtol=0, atol=1e-12)


@pytest.mark.parametrize("concat", [True, False])
def test_restatement_equals_masked_scaled_dot_product_attention(concat):
    """A duplicate-free graph in which every node has an in-edge: the layer without its root term is torch's
    scaled_dot_product_attention of its projections under the adjacency as a boolean mask (H = 2, C = 8)."""
    n, f, H, C = 30, 6, 2, 8
    g = torch.Generator().manual_seed(5)
    adj = torch.rand((n, n), generator=g) < 0.2                       # adj[i, j]: edge j -> i
    adj[torch.arange(n), (torch.arange(n) + 1) % n] = True            # every row has an in-edge
    adj[3, 3] = adj[7, 7] = True                                      # self-loops stay
    dst, src = adj.nonzero(as_tuple=True)
    ei = torch.stack([src, dst])[:, torch.randperm(src.numel(), generator=g)]
    x = torch.randn(n, f, generator=g, dtype=torch.float64)
    conv = RefTransformerConv(f, C, heads=H, concat=concat, root_weight=False).eval()
    got = conv(x, ei)
    heads = lambda lin: lin(x).view(n, H, C).transpose(0, 1)          # [H, n, C]
    want = F.scaled_dot_product_attention(heads(conv.lin_query), heads(conv.lin_key), heads(conv.lin_value),
                                          attn_mask=adj).transpose(0, 1)
    want = want.reshape(n, H * C) if concat else want.mean(1)
    assert (got - want).abs().max().item() < 1e-12


def test_root_and_beta_follow_the_formulas():
    x, ei, ref = layer_case("beta")
    ref.eval()
    n, H, C = x.size(0), ref.H, ref.C
    out = ref(x, ei)
    att, _ = attend(ref.lin_query(x).view(n, H, C), ref.lin_key(x).view(n, H, C), ref.lin_value(x).view(n, H, C), n,
                    ei[0], ei[1], 1.0 / math.sqrt(C))
    att, x_r = att.reshape(n, H * C), ref.lin_skip(x)
    w = ref.lin_beta.weight[0]
    b = torch.sigmoid(att @ w[:16] + x_r @ w[16:32] + (att - x_r) @ w[32:]).unsqueeze(1)
    assert (out - (b * x_r + (1 - b) * att)).abs().max().item() < 1e-12
    ref.lin_beta = None
    assert (ref(x, ei) - (att + x_r)).abs().max().item() < 1e-12
    no_in = torch.bincount(ei[1], minlength=n) == 0
    assert bool(no_in.any()) and att[no_in].abs().max().item() == 0.0   # the layer case has nodes without in-edges


# ---- registry, module layout, refusals ---------------------------------------------------------------------------------------

def test_registry():
    from rgb_experiment_amd.dist import experiment as dist_experiment
    from rgb_experiment_amd.models import MODELS, REGISTRY, GraphTransformer
    assert MODELS["transformer"] is GraphTransformer and "transformer" not in REGISTRY
    assert "transformer" not in dist_experiment.SUPPORTED


def pyg_shaped_state(f, C, H, concat, beta, root_weight, bias):
    """Names and shapes of PyG's TransformerConv.state_dict() for these keywords."""
    wide, skip = H * C, H * C if concat else C
    shapes = {}
    for name in ("lin_key", "lin_query", "lin_value"):
        shapes[name + ".weight"], shapes[name + ".bias"] = (wide, f), (wide,)
    shapes["lin_skip.weight"] = (skip, f)
    if bias:
        shapes["lin_skip.bias"] = (skip,)
    if beta and root_weight:
        shapes["lin_beta.weight"] = (1, 3 * skip)
    return shapes


@pytest.mark.parametrize("concat,beta,root_weight,bias", list(itertools.product([True, False], repeat=4)))
def test_state_dict_layout_and_strict_loading(concat, beta, root_weight, bias):
    from rgb_experiment_amd.nn import TransformerConv
    kw = dict(concat=concat, beta=beta, root_weight=root_weight, bias=bias)
    conv = TransformerConv(6, 4, heads=3, **kw)
    shapes = pyg_shaped_state(6, 4, 3, **kw)
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == shapes
    assert (conv.lin_beta is not None) == (beta and root_weight) and conv.beta == (beta and root_weight)
    g = torch.Generator().manual_seed(1)
    state = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    conv.load_state_dict(state, strict=True)
    ref = RefTransformerConv(6, 4, heads=3, **kw)
    ref.load_state_dict({k: v.double() for k, v in state.items()}, strict=True)
    assert sorted(dict(conv.named_parameters())) == sorted(dict(ref.named_parameters()))


def test_model_layout():
    from rgb_experiment_amd.models import GraphTransformer
    from rgb_experiment_amd.nn import TransformerConv
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    for kw in (dict(), dict(beta=True), dict(root_weight=False)):
        model = GraphTransformer(3, 4, 10, 5, 0.5, 2, **kw)
        first, last = model.convs[0], model.convs[-1]
        assert isinstance(first, TransformerConv) and first.heads == 2 and first.concat
        assert last.heads == 1 and not last.concat and len(model.bns) == 2
        assert shapes(model)["convs.1.lin_key.weight"] == (8, 8) and shapes(model)["convs.2.lin_skip.weight"] == (5, 8)
        assert ("convs.2.lin_beta.weight" in shapes(model)) == bool(kw.get("beta"))
        ref = RefGraphTransformer(3, 4, 10, 5, 2, **kw)
        ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()},
                            strict=True)
        model.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()},
                              strict=True)
    assert GraphTransformer(2, 4, 10, 5, 0.5, 2, att_dropout=0.25).convs[1].dropout == 0.25


def test_refusals():
    import rgb_experiment_amd as R
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.nn import TransformerConv
    with pytest.raises(NotImplementedError, match="edge_dim"):
        TransformerConv(4, 4, edge_dim=3)
    for p in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="dropout"):
            TransformerConv(4, 4, dropout=p)
    conv = TransformerConv(4, 3, heads=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(torch.randn(5, 4), torch.tensor([[0, 1], [1, 2]]))

    class Partitioned:
        is_distributed = True
    t = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="no node-partitioned form"):
        ops.transformer_attend(t, t, t, Partitioned(), 2, 4, 0.5)
    g = torch.Generator().manual_seed(0)
    data = R.Data(x=torch.randn(30, 6, generator=g), y=torch.randint(0, 3, (30,), generator=g),
                  edge_index=torch.randint(0, 30, (2, 90), generator=g))
    params = {"num_layers": 2, "hidden_unit": 4, "dropout_rate": 0.0, "heads": 2}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.experiment(params, specify_data=True, data=data, model_name="transformer", use_cpu=True, print_print=False)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------

NEW_ENTRIES = ("rgbx_transformer_supported", "rgbx_transformer_fwd_f32", "rgbx_transformer_bwd_dst_f32",
               "rgbx_transformer_bwd_src_f32")


def test_abi_declares_and_exports_the_new_entries():
    from rgb_experiment_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbx_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rgbx_[a-z0-9_]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS, name
        # one ctypes argument per declared parameter
        params = re.search(name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(_lib.SIGNATURES[name]) == len([a for a in params.split(",") if a.strip()]), name
    assert not any(n.startswith("rgbx_transformer_draws") for n in declared)   # rgbx_gatv2_draws_u8 serves
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.rgbx_version() == 501
    p = 0x10000  # 16-byte aligned, non-null, never dereferenced: every call below returns before a launch
    ok = lib.rgbx_transformer_supported
    for H, C in PAIRS + [(1, 128), (2, 66)]:
        assert ok(H, C) and lib.rgbx_gatv2_supported(H, C)
    for H, C in [(1, 67), (2, 67), (1, 130), (1, 260), (0, 8), (8, 0)]:
        assert not ok(H, C) and not lib.rgbx_gatv2_supported(H, C)

    def fwd(**kw):
        a = dict(rowptr=p, q=p, ldq=64, k=p, v=p, ldv=64, out=p, m=p, rden=p, N=10, H=8, C=8, scale=0.35, seed=None,
                 p_drop=0.0)
        a.update(kw)
        return lib.rgbx_transformer_fwd_f32(a["rowptr"], p, a["q"], a["ldq"], a["k"], 64, a["v"], a["ldv"], a["out"], 64,
                                            a["m"], a["rden"], a["N"], a["H"], a["C"], a["scale"], a["seed"], a["p_drop"],
                                            None, None)
    assert fwd(rowptr=None) == -1 and b"null" in lib.rgbx_last_error_string()
    assert fwd(q=None) == -1 and fwd(k=None) == -1 and fwd(v=None) == -1 and fwd(out=None) == -1
    assert fwd(ldq=32) == -1 and fwd(ldv=63) == -1           # leading dimension < H*C
    assert fwd(m=None) == -1                                 # m without rden
    assert fwd(m=None, rden=None, seed=p) == -1              # the inference form has no dropout
    assert fwd(seed=p, p_drop=1.0) == -1
    assert fwd(scale=0.0) == -1 and fwd(scale=float("nan")) == -1 and b"scale" in lib.rgbx_last_error_string()
    assert fwd(N=-1) == -1 and fwd(H=0) == -1
    assert fwd(N=2 ** 31) == -2
    assert fwd(H=1, C=67, ldq=67) == -5 and fwd(H=1, C=1000, ldq=1000) == -5   # RGBX_E_SHAPE
    assert fwd(v=p + 2) == -3 and b"aligned" in lib.rgbx_last_error_string()   # RGBX_E_ALIGN
    assert fwd(N=0) == 0                                     # nothing to do

    def dst(**kw):
        a = dict(k=p, m=p, out=p, ldg=64, nodeq=p, g_q=p, ldgq=64, N=1000, C=8, scale=0.35, seed=None, p_drop=0.0)
        a.update(kw)
        return lib.rgbx_transformer_bwd_dst_f32(p, p, p, 64, a["k"], 64, p, 64, a["m"], p, a["out"], 64, p, a["ldg"],
                                                a["nodeq"], a["g_q"], a["ldgq"], a["N"], 8, a["C"], a["scale"], a["seed"],
                                                a["p_drop"], None, None)
    assert dst(k=None) == -1 and dst(m=None) == -1 and dst(out=None) == -1 and dst(g_q=None) == -1
    assert dst(nodeq=None) == -1
    assert dst(ldg=32) == -1 and dst(ldgq=63) == -1
    assert dst(nodeq=p + 4) == -3                            # the record is written as 8-byte pairs
    assert dst(k=p + 1) == -3
    assert dst(C=67) == -5
    assert dst(seed=p, p_drop=-0.5) == -1
    assert dst(scale=-1.0) == -1
    assert dst(N=2 ** 31) == -2 and dst(N=0) == 0

    def src(**kw):
        a = dict(t2f=None, q=p, v=p, ldgk=64, ldgv=64, nodeq=p, g_k=p, g_v=p, N=1000, C=8, scale=0.35, seed=None,
                 p_drop=0.0)
        a.update(kw)
        return lib.rgbx_transformer_bwd_src_f32(p, p, a["t2f"], a["q"], 64, p, 64, a["v"], 64, a["nodeq"], p, 64, a["g_k"],
                                                a["ldgk"], a["g_v"], a["ldgv"], a["N"], 8, a["C"], a["scale"], a["seed"],
                                                a["p_drop"], None, None)
    assert src(q=None) == -1 and src(v=None) == -1 and src(g_k=None) == -1 and src(g_v=None) == -1
    assert src(nodeq=None) == -1
    assert src(ldgk=63) == -1 and src(ldgv=32) == -1
    assert src(seed=p, p_drop=0.5) == -1 and b"slot map" in lib.rgbx_last_error_string()
    assert src(nodeq=p + 4) == -3 and src(g_v=p + 2) == -3
    assert src(C=130) == -5
    assert src(scale=float("inf")) == -1
    assert src(N=0) == 0


# ---- preconditions of the GPU cases ---------------------------------------------------------------------------------------------

def test_graphs_have_what_the_cases_need():
    from rgb_experiment_amd import graph as G
    assert G.LONG_ROW_SLOTS == LONG_ROW_SLOTS
    ei, n = graph_of("random")
    indeg, outdeg = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
    assert int((indeg == 0).sum()) >= 20 and int((outdeg == 0).sum()) >= 20
    assert int((ei[0] == ei[1]).sum()) > 0
    assert torch.unique(ei[0] * n + ei[1]).numel() < ei.size(1)       # duplicates
    ei, n = graph_of("powerlaw")
    assert int(torch.bincount(ei[1], minlength=n).max()) > LONG_ROW_SLOTS
    assert int(torch.bincount(ei[0], minlength=n).max()) > LONG_ROW_SLOTS
    assert graph_of("no_edges")[0].size(1) == 0


@pytest.mark.parametrize("graph", GRAPH_NAMES)
@pytest.mark.parametrize("H,C", PAIRS)
def test_operator_case_is_well_posed(H, C, graph):
    """Eval mode and p = 0.5 with synthetic decisions: float32 on the CPU stays inside a quarter of the tolerance."""
    case = operator_case(H, C, graph)
    src, dst, _, _ = slots_of(graph)
    want = eval_reference(H, C, graph)
    low = run_formula(case, graph, H, C, torch.float32)
    shares = shares_of(low, want)
    keep = synthetic_keep(src.numel(), H, 3)
    want_d = run_formula(case, graph, H, C, keep=keep, p=0.5)
    low_d = run_formula(case, graph, H, C, torch.float32, keep=keep, p=0.5)
    shares_d = shares_of(low_d, want_d)
    print(f"({H}, {C}) {graph}: max |e| {want[2].abs().max().item() if want[2].numel() else 0.0:.1f}; float32 vs float64 "
          f"share of tolerance, eval {shares}, dropout {shares_d}")
    assert all(torch.isfinite(t).all() for t in [low[0]] + low[1] + [low_d[0]] + low_d[1])
    assert max(shares.values()) <= WELL_POSED_SHARE and max(shares_d.values()) <= WELL_POSED_SHARE
    if graph == "no_edges":
        assert all(t.abs().max().item() == 0.0 for t in [want[0]] + want[1])


@pytest.mark.parametrize("graph", LARGE_GRAPHS)
@pytest.mark.parametrize("H,C", LARGE_PAIRS)
def test_large_case_is_in_range_and_well_posed(H, C, graph):
    """The scores overflow an unshifted expf (|e| > 90), `powerlaw` shows late maxima in long rows and hub-row chunks with
    maxima far apart, and float32 stays inside a quarter of the unchanged tolerance."""
    case = large_case(H, C, graph)
    want = eval_reference(H, C, graph, large=True)
    prof = score_profile(want[2], graph)
    low = run_formula(case, graph, H, C, torch.float32)
    shares = shares_of(low, want)
    print(f"large ({H}, {C}) {graph}: max |e| {prof['max_abs']:.1f}, {int((want[2].abs() > 90).sum())} scores beyond 90, "
          f"late-maximum rows {prof['late_rows']}, hub maxima in chunks {sorted(prof['chunks'])}; float32 vs float64 share "
          f"of tolerance {shares}")
    assert prof["max_abs"] > 90 and int((want[2].abs() > 90).sum()) >= 10
    assert not bool(torch.isfinite(torch.exp(want[2].float())).all())      # the unshifted float32 form overflows
    if graph == "powerlaw":
        assert prof["late_rows"] >= 20
        assert prof["chunks"] >= ({"first", "last"} if H >= 2 else {"last"})
    assert all(torch.isfinite(t).all() for t in [low[0]] + low[1])
    assert max(shares.values()) <= WELL_POSED_SHARE, shares


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("name", sorted(LAYER_CASES))
def test_layer_case_is_well_posed(name, train):
    H, C, _ = LAYER_CASES[name]
    p = 0.5 if train else 0.0
    x, ei, ref = layer_case(name, p)
    ref.train(train)
    choices = {"src": ei[0], "dst": ei[1], "keep": synthetic_keep(ei.size(1), H, 4)} if train else None
    cot = f32_exact((LAYER_N, ref.lin_skip.weight.size(0)), torch.Generator().manual_seed(17))
    low = copy.deepcopy(ref).float()
    shares = {}
    x64, x32 = x.clone().requires_grad_(True), x.float().requires_grad_(True)
    want, got = ref(x64, ei, choices), low(x32, ei, choices)
    (want * cot).sum().backward()
    (got * cot.float()).sum().backward()
    shares["forward"] = share_of_tolerance(got, want, FWD_TOL)
    shares["x"] = share_of_tolerance(x32.grad, x64.grad, GRAD_TOL)
    lowp = dict(low.named_parameters())
    for key, prm in ref.named_parameters():
        if prm.grad is None:
            assert key.startswith("lin_skip") and not ref.root_weight and lowp[key].grad is None
            continue
        shares[key] = share_of_tolerance(lowp[key].grad, prm.grad, GRAD_TOL)
    print(f"{name} train={train}: {shares}")
    assert max(shares.values()) <= WELL_POSED_SHARE, shares


@pytest.mark.parametrize("kw", [dict(), dict(beta=True)], ids=["plain", "beta"])
def test_model_case_is_well_posed(kw):
    x, y, ei, model, ref = model_case(**kw)
    ref.train()
    low = copy.deepcopy(ref).float()
    want, got = ref(x, ei), low(x.float(), ei)
    F.nll_loss(want["out"], y).backward()
    F.nll_loss(got["out"], y).backward()
    shares = {"emb": share_of_tolerance(got["emb"], want["emb"], FWD_TOL),
              "out": share_of_tolerance(got["out"], want["out"], FWD_TOL)}
    lowp = dict(low.named_parameters())
    for key, prm in ref.named_parameters():
        shares[key] = share_of_tolerance(lowp[key].grad, prm.grad, GRAD_TOL)
    print(shares)
    assert max(shares.values()) <= WELL_POSED_SHARE, shares
