"""FiLMConv on the host: a float64 restatement of the layer, written PER RELATION WITH MASKS (for every relation r the
edges of that relation are selected, their messages act(gamma_r[i] * h_r[j] + beta_r[i]) summed per target and divided by
their count), not with CSR slots and slot weights as the product computes it; pinned by numbers derived by hand on a
planted graph. Registry, module layout (PyG's names, strict state_dict loading both ways, a custom `nn`), refusals of the
layer, the op and experiment(), the C ABI of the new entry points; and the case builders tests/test_gpu_film.py feeds to
the HIP kernels, with the checks that keep those cases well-posed. No GPU needed.

Well-posedness. The message has a kink (relu), so a case is only a fair comparison if float32 and float64 agree on the
mask. OPERATOR cases draw h, fb, y0 and the cotangent from the dyadic grid k / 8: gamma * h + beta is then EXACT in
float32 (asserted per slot and channel), with or without a fused multiply-add, so the mask is the same in both
precisions. h and gamma are ODD multiples of 1 / 8 and beta any multiple: the sum is an odd multiple of 1 / 64 and
never zero, except at the planted ties (gamma = 2, h = 0.5, beta = -1), which are the only zeros (asserted). What is left
is summation error: every case is run through the restatement in float32 on the CPU with the edges and the relations in
REVERSED order and has to stay within a QUARTER (WELL_POSED_SHARE) of the GPU test's tolerances (forward 1e-4, gradients
2e-4, times max(1, |ref|max)) of the float64 result. LAYER and MODEL cases compute h and fb by float32 dot products, so
there no relu input of the float64 run may lie within a margin of zero: the float32 dot-product error bound (as
relu_margin in tests/test_gine_host.py), carried through the film product and, in the model, BatchNorm. Seeds are fixed
so that this holds; a case that does not satisfy it fails, it is never skipped."""
import copy
import functools
import inspect
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from rgb_experiment_amd.models import FiLM              # without the feature this file fails here, at import
from rgb_experiment_amd.nn import FiLMConv

import test_gine_host as G
import test_rgcn_host as RG
from test_transformer_host import FWD_TOL, GRAD_TOL, LONG_ROW_SLOTS, WELL_POSED_SHARE, f32_exact, share_of_tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32, gamma_k = G.U32, G.gamma


# ---- the restatement ---------------------------------------------------------------------------------------------------

def activation(z, act):
    if act == "relu":
        return torch.relu(z)                               # torch's derivative at 0 is 0
    if act in (None, "identity"):
        return z
    raise ValueError(act)


def aggregate(rows, beta, gamma, n, src, dst, et, aggr="mean", act="relu", reverse=False):
    """out [n, C] = sum over the relations r of AGG over the edges (src -> dst) of relation r, as given, of
    act(gamma[r, dst] * rows[r, src] + beta[r, dst]); rows / beta / gamma [R, n, C] hold the message row of every
    (relation, source) and the film rows of every (relation, target). AGG is the mean per (target, relation) — the sum
    divided by the number of edges of relation r into the target, duplicates counted — or the sum with aggr="add". A
    (target, relation) pair without an edge contributes 0. `reverse`: relations and edges backwards."""
    R, _, C = rows.shape
    out = torch.zeros(n, C, dtype=rows.dtype)
    for r in (reversed(range(R)) if reverse else range(R)):
        mine = (et == r).nonzero(as_tuple=True)[0]
        if reverse:
            mine = mine.flip(0)
        s, d = src[mine], dst[mine]
        m = activation(gamma[r].index_select(0, d) * rows[r].index_select(0, s) + beta[r].index_select(0, d), act)
        tot = torch.zeros(n, C, dtype=rows.dtype).index_add(0, d, m)
        if aggr == "mean":
            tot = tot / torch.bincount(d, minlength=n).clamp(min=1).to(rows.dtype)[:, None]
        elif aggr not in ("add", "sum"):
            raise ValueError(aggr)
        out = out + tot
    return out


def film_rows(h, fb, R):
    """(rows, beta, gamma), each [R, n, C], from h [n, R * C] (column block r: the messages under relation r) and fb
    [n, R * 2C] (column block r: beta_r | gamma_r, beta FIRST)."""
    n = h.size(0)
    C = h.size(1) // R
    f = fb.view(n, R, 2 * C)
    return h.view(n, R, C).permute(1, 0, 2), f[:, :, :C].permute(1, 0, 2), f[:, :, C:].permute(1, 0, 2)


class RefFiLMConv(nn.Module):
    """float64 restatement of FiLMConv with PyG's module names: lins[r] = Linear(in, out, bias=False), films[r] =
    Linear(in, 2 * out) or a deep copy of `net`, lin_skip = Linear(in, out, bias=False), film_skip = Linear(in, 2 * out,
    bias=False) or a deep copy of `net`. Keeps the relu inputs of its last forward (`relu_inputs`: per relation, then
    the skip term)."""

    def __init__(self, in_channels, out_channels, num_relations=1, net=None, act="relu", aggr="mean"):
        super().__init__()
        self.C, self.R, self.act, self.aggr = out_channels, num_relations, act, aggr
        film = lambda bias: copy.deepcopy(net) if net is not None else nn.Linear(in_channels, 2 * out_channels, bias=bias)
        self.lins = nn.ModuleList(nn.Linear(in_channels, out_channels, bias=False) for _ in range(num_relations))
        self.films = nn.ModuleList(film(True) for _ in range(num_relations))
        self.lin_skip = nn.Linear(in_channels, out_channels, bias=False)
        self.film_skip = film(False)
        self.double()
        self.relu_inputs = []

    def forward(self, x, ei, et=None, reverse=False):
        n, C = x.size(0), self.C
        et = torch.zeros(ei.size(1), dtype=torch.int64) if et is None or self.R == 1 else et
        beta_s, gamma_s = self.film_skip(x).split(C, dim=-1)
        z_skip = gamma_s * self.lin_skip(x) + beta_s
        rows = torch.stack([lin(x) for lin in self.lins])
        fb = [film(x).split(C, dim=-1) for film in self.films]
        beta, gamma = torch.stack([b for b, _ in fb]), torch.stack([g for _, g in fb])
        self.relu_inputs = [(gamma[r][ei[1][et == r]] * rows[r][ei[0][et == r]] + beta[r][ei[1][et == r]]).detach()
                            for r in range(self.R)] + [z_skip.detach()]
        return activation(z_skip, self.act) + aggregate(rows, beta, gamma, n, ei[0], ei[1], et, self.aggr, self.act,
                                                        reverse)


class RefFiLM(nn.Module):
    """models/film.py in float64: num_layers FiLMConv layers, BatchNorm and dropout behind every layer but the last,
    which has act=None; the product's names. Keeps the input of every conv of its last forward (`conv_inputs`)."""

    def __init__(self, input_dim, output_dim, hidden_unit, num_layers, dropout_rate, num_relations=1, aggr="mean"):
        super().__init__()
        self.dropout_rate = dropout_rate
        dims = [input_dim] + [hidden_unit] * (num_layers - 1) + [output_dim]
        last = len(dims) - 2
        self.convs = nn.ModuleList(RefFiLMConv(a, b, num_relations, act=None if i == last else "relu", aggr=aggr)
                                   for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])))
        self.norms = nn.ModuleList(nn.BatchNorm1d(hidden_unit).double() for _ in range(num_layers - 1))
        self.conv_inputs = []

    def forward(self, x, ei, et=None, reverse=False):
        self.conv_inputs = []
        for conv, norm in zip(self.convs[:-1], self.norms):
            self.conv_inputs.append(x.detach())
            x = F.dropout(norm(conv(x, ei, et, reverse)), p=self.dropout_rate, training=self.training)
        self.conv_inputs.append(x.detach())
        x = self.convs[-1](x, ei, et, reverse)
        return {"out": F.log_softmax(x, dim=1), "emb": x}


def randomize(module, seed):
    """Every parameter of a reference module set to fp32-exact random values: weights N(0, 1 / fan_in), the rest
    N(0, 0.5)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            p.copy_(f32_exact(tuple(p.shape), g, p.size(-1) ** -0.5 if p.dim() == 2 else 0.5))
    return module


# ---- graphs and edge types --------------------------------------------------------------------------------------------

graph_names = RG.graph_names                                # no_edges, random, powerlaw, degrees, n1, n2, n3
RELATIONS = (1, 3, 7)
PLANTED_R = RG.PLANTED_R
graph_of, slots_of = RG.graph_of, RG.slots_of               # `planted` included


@functools.lru_cache(maxsize=None)
def edge_type_of(name, R):
    """tests/test_rgcn_host.edge_type_of (int64 [E], seeded; with R > 1 the LAST relation owns no edge), except on
    `degrees` with R > 1: there every edge takes the relation k % (R - 1) of its hub endpoint k (the target k < 6 of
    DEGREES[k] in-edges, the source 6 + k of DEGREES[k] out-edges), so that the rows of exactly 0 / 1 / 64 / 65 / T / T + 1
    slots exist in the two relation-expanded CSRs as well; the nodes from 12 on still receive a mix of relations."""
    if name == "degrees" and R > 1:
        ei, _ = graph_of(name)
        hub = torch.where(ei[1] < 6, ei[1], ei[0] - 6)
        assert int(hub.min()) >= 0 and int(hub.max()) < 6
        return hub % (R - 1)
    return RG.edge_type_of(name, R)


# ---- operator cases shared with tests/test_gpu_film.py ----------------------------------------------------------------

WIDTHS = [1, 4, 7, 16, 64, 66]          # vector widths 1 (1, 7), 2 (66) and 4 (4, 16, 64)
PADDED_WIDTH = 67                       # outside the layout: the layer pads it to 68
BLOCKED_WIDTH = 300                     # above 256: column blocks of 256 and 44
TIE_EVERY = 7                           # every 7th edge carries one planted tie
NAMES = ("forward", "g_h", "g_fb", "g_y0")
# (C, R, graph, aggr, act). Every (C, R) on `degrees`; one width per vector width on the hub-row graph, under every R;
# add and identity on both; the small graphs, the graph without edges and the planted graph.
CASES = ([(C, R, "degrees", "mean", "relu") for C in WIDTHS for R in RELATIONS]
         + [(C, R, "powerlaw", "mean", "relu") for C in (7, 64, 66) for R in RELATIONS]
         + [(C, R, g, aggr, act) for (C, R) in ((7, 3), (64, 1), (66, 7)) for g in ("degrees", "powerlaw")
            for aggr, act in (("add", "relu"), ("mean", "identity"), ("add", "identity"))]
         + [(C, R, g, "mean", "relu") for (C, R) in ((7, 3), (4, 1)) for g in ("no_edges", "random") + G.SMALL_GRAPHS]
         + [(4, PLANTED_R, "planted", aggr, act) for aggr in ("mean", "add") for act in ("relu", "identity")]
         + [(BLOCKED_WIDTH, 3, "random", "mean", "relu"), (BLOCKED_WIDTH, 1, "random", "add", "relu")])


def _grid(shape, gen, odd=False):
    """Multiples of 1 / 8 in [-2, 2] (float64); `odd`: odd multiples in [-15 / 8, 15 / 8]."""
    if odd:
        return (2 * torch.randint(-8, 8, shape, generator=gen) + 1).double() / 8
    return torch.randint(-16, 17, shape, generator=gen).double() / 8


def tie_positions(n_edges, C):
    k = torch.arange(0, n_edges, TIE_EVERY)
    return k, (k // TIE_EVERY) % C


# the planted graph's tables, one channel: h[j, r] = HJ[j] + r; (gamma, beta) of the (target, relation) pairs that
# own an edge (every other pair: gamma 1, beta 0); y0
PLANTED_HJ = (0.5, 1.0, 1.5, 2.0, 2.5, 3.0)
PLANTED_FILM = {(0, 0): (-1.0, 1.75), (1, 0): (2.0, -1.0), (1, 1): (1.0, 0.5), (1, 2): (0.5, -3.0), (2, 1): (2.0, 1.0),
                (2, 0): (-2.0, 6.0), (3, 2): (0.25, 0.0)}
PLANTED_Y0 = (10.0, 20.0, 30.0, 40.0, 50.0, 60.0)


def planted_tables(C):
    """(rows, beta, gamma) [n, R, C] of the planted graph, every channel the same."""
    n, R = 6, PLANTED_R
    rows = torch.tensor(PLANTED_HJ, dtype=torch.float64)[:, None] + torch.arange(R, dtype=torch.float64)[None, :]
    gamma, beta = torch.ones(n, R, dtype=torch.float64), torch.zeros(n, R, dtype=torch.float64)
    for (i, r), (g, b) in PLANTED_FILM.items():
        gamma[i, r], beta[i, r] = g, b
    rep = lambda t: t[:, :, None].repeat(1, 1, C)
    return rep(rows), rep(beta), rep(gamma)


@functools.lru_cache(maxsize=4)
def operator_case(C, R, graph_name):
    """(h [n, R * C], fb [n, R * 2C], y0 [n, C], cotangent [n, C], tie mask [E, C]): float64 on the grid k / 8. h and gamma
    are odd multiples, so gamma * h + beta is an odd multiple of 1 / 64: never zero. Every TIE_EVERY-th edge e = (j -> i)
    of relation r plants, in one channel c, gamma[i, r, c] = 2, beta[i, r, c] = -1 and h[j, r, c] = 0.5: z = 0 there, and
    wherever else a planted film entry meets a planted h entry over an edge; nowhere else. The planted graph carries
    its hand-made tables on every channel."""
    ei, n = graph_of(graph_name)
    et = edge_type_of(graph_name, R)
    g = torch.Generator().manual_seed(5000 + 100 * R + C)
    if graph_name == "planted":
        rows, beta, gamma = planted_tables(C)
    else:
        rows, gamma, beta = _grid((n, R, C), g, odd=True), _grid((n, R, C), g, odd=True), _grid((n, R, C), g)
        k, c = tie_positions(ei.size(1), C)
        gamma[ei[1][k], et[k], c], beta[ei[1][k], et[k], c], rows[ei[0][k], et[k], c] = 2.0, -1.0, 0.5
    if graph_name == "planted":
        y0 = torch.tensor(PLANTED_Y0, dtype=torch.float64)[:, None].repeat(1, C)
    else:
        y0 = _grid((n, C), g)
    cot = _grid((n, C), g)
    ties = (gamma[ei[1], et] == 2.0) & (beta[ei[1], et] == -1.0) & (rows[ei[0], et] == 0.5)   # [E, C]
    return rows.reshape(n, R * C), torch.cat([beta, gamma], dim=2).reshape(n, R * 2 * C), y0, cot, ties


def run_formula(case, R, graph_name, aggr, act, dtype=torch.float64, reverse=False):
    """The restatement on an operator case in `dtype`: (out, [g_h, g_fb, g_y0])."""
    ei, n = graph_of(graph_name)
    h, fb, y0 = (t.to(dtype).clone().requires_grad_(True) for t in case[:3])
    rows, beta, gamma = film_rows(h, fb, R)
    out = y0 + aggregate(rows, beta, gamma, n, ei[0], ei[1], edge_type_of(graph_name, R), aggr, act, reverse)
    (out * case[3].to(dtype)).sum().backward()
    return out.detach(), [h.grad, fb.grad, y0.grad]


@functools.lru_cache(maxsize=4)
def reference(C, R, graph_name, aggr, act):
    """The float64 result of a case, computed once and shared (read-only) by the host and the GPU tests."""
    return run_formula(operator_case(C, R, graph_name), R, graph_name, aggr, act)


def shares_of(got, want):
    out = {NAMES[0]: share_of_tolerance(got[0], want[0], FWD_TOL)}
    for name, a, b in zip(NAMES[1:], got[1], want[1]):
        assert a.shape == b.shape
        out[name] = share_of_tolerance(a, b, GRAD_TOL)
    return out


def slot_inputs(case, R, graph_name):
    """(gamma, h, beta) of every (edge, channel), each [E, C] float64: the three operands of the message's fmaf."""
    ei, n = graph_of(graph_name)
    et = edge_type_of(graph_name, R)
    rows, beta, gamma = (t.permute(1, 0, 2) for t in film_rows(case[0], case[1], R))   # [n, R, C]
    return gamma[ei[1], et], rows[ei[0], et], beta[ei[1], et]


def check_masks_agree(case, R, graph_name):
    """gamma * h + beta is exact in float32 in every slot and channel — the product alone too, so fused and unfused
    arithmetic give the same number — and its zeros are exactly the planted ties. -> the number of ties."""
    g, h, b = slot_inputs(case, R, graph_name)
    prod64, z64 = g * h, g * h + b                          # exact: a handful of bits each
    prod32 = g.float() * h.float()
    assert torch.equal(prod32.double(), prod64) and torch.equal((prod32 + b.float()).double(), z64)
    assert torch.equal(torch.addcmul(b.float(), g.float(), h.float()).double(), z64)
    assert torch.equal(z64 == 0, case[4])
    return int(case[4].sum())


# ---- layer and model cases ----------------------------------------------------------------------------------------------

def linear_bound(mod, x, x_err):
    """(value, err) of a Linear — or a Sequential of Linears — of the reference on a float64 input that arrives with
    an error of at most `x_err` (a number or a tensor like x): |float32 result - value| <= err for any order of the dot
    product's sum, with or without fused multiply-adds: gamma(D + 1) (|x| |W|^T + |b|), plus the input's error carried
    through |W|."""
    if isinstance(mod, nn.Sequential):
        val, err = x, x_err
        for layer in mod:
            val, err = linear_bound(layer, val, err)
        return val, err
    assert isinstance(mod, nn.Linear)
    W = mod.weight.detach().abs()
    mag = x.detach().abs() @ W.t() + (0 if mod.bias is None else mod.bias.detach().abs())
    carried = x_err @ W.t() if torch.is_tensor(x_err) else x_err * W.sum(1)
    return mod(x).detach(), gamma_k(mod.in_features + 1) * mag + carried


def relu_margins(conv, x, ei, et=None, x_err=0.0):
    """Per relation, then for the skip term: (z, margin) with z the float64 relu input of every (edge, channel) — (node,
    channel) for the skip term — and margin an upper bound of |float32 z - float64 z|: with the errors eg, eh, eb of
    gamma, h, beta (linear_bound), |dz| <= eg (|h| + eh) + |g| eh + eb, plus the roundings of the product and the add,
    2 u (|g h| + |b|), which covers the fused form (one rounding) too."""
    C = conv.C
    et = torch.zeros(ei.size(1), dtype=torch.int64) if et is None or conv.R == 1 else et
    out = []
    parts = [(conv.lins[r], conv.films[r], ei[0][et == r], ei[1][et == r]) for r in range(conv.R)]
    every = torch.arange(x.size(0))
    parts.append((conv.lin_skip, conv.film_skip, every, every))
    for lin, film, s, d in parts:
        h, eh = linear_bound(lin, x, x_err)
        f, ef = linear_bound(film, x, x_err)
        (b, g), (eb, eg) = f.split(C, dim=-1), ef.split(C, dim=-1)
        z = g[d] * h[s] + b[d]
        margin = eg[d] * (h[s].abs() + eh[s]) + g[d].abs() * eh[s] + eb[d] + 2 * U32 * ((g[d] * h[s]).abs() + b[d].abs())
        out.append((z, margin))
    return out


LAYER_N, LAYER_E, LAYER_F, LAYER_R = 80, 500, 6, 3


def custom_net(C):
    """A caller's film network: two Linears, so film_skip (a copy) carries biases the default has not."""
    return nn.Sequential(nn.Linear(LAYER_F, 5), nn.Linear(5, 2 * C))


LAYER_CASES = {   # name -> (out_channels, num_relations, custom nn?, layer keywords, parameter seed)
    "typed": (7, LAYER_R, False, dict(), 44),
    "typed_add": (7, LAYER_R, False, dict(aggr="add"), 44),
    "typed_identity": (16, LAYER_R, False, dict(act=None), 44),
    "typed_padded": (PADDED_WIDTH, LAYER_R, False, dict(), 44),
    "one_relation": (7, 1, False, dict(), 44),
    "one_relation_sum": (66, 1, False, dict(aggr="sum", act="identity"), 44),
    "custom_nn": (7, LAYER_R, True, dict(), 45),
    "custom_nn_padded": (PADDED_WIDTH, 1, True, dict(), 44),
}


def layer_case(name):
    """(x float64 fp32-exact, edge_index, edge_type or None, reference layer with fp32-exact random parameters)."""
    from test_gpu_ggnn import rand_graph
    C, R, custom, kw, seed = LAYER_CASES[name]
    ei = rand_graph(LAYER_N, LAYER_E, 41, loops=5, dups=12)
    ei = ei[:, ei[1] >= 5].contiguous()                                    # nodes 0 .. 4 keep no in-edge: out == skip term
    et = torch.randint(0, R, (ei.size(1),), generator=torch.Generator().manual_seed(42)) if R > 1 else None
    x = f32_exact((LAYER_N, LAYER_F), torch.Generator().manual_seed(43))
    ref = randomize(RefFiLMConv(LAYER_F, C, R, net=custom_net(C) if custom else None, **kw), seed)
    return x, ei, et, ref


def product_layer(name, ref):
    """The product's layer (on the CPU) holding the reference's parameters."""
    C, R, custom, kw, _ = LAYER_CASES[name]
    conv = FiLMConv(LAYER_F, C, R, nn=custom_net(C) if custom else None, **kw)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return conv


MODEL_SHAPE = dict(n=60, e=300, f=16, hidden=12, classes=5, layers=3)
MODEL_RELATIONS = (1, 4)


def model_case(R):
    """(x, y, edge_index, edge_type or None, the product's model on the CPU, the reference holding the same parameters)."""
    from test_gpu_ggnn import rand_graph
    s = MODEL_SHAPE
    g = torch.Generator().manual_seed(51)
    ei = rand_graph(s["n"], s["e"], 52, loops=4, dups=6)
    et = torch.randint(0, R, (ei.size(1),), generator=g) if R > 1 else None
    x, y = f32_exact((s["n"], s["f"]), g), torch.randint(0, s["classes"], (s["n"],), generator=g)
    ref = randomize(RefFiLM(s["f"], s["classes"], s["hidden"], s["layers"], 0.0, R), 53)
    model = FiLM(s["f"], s["classes"], s["hidden"], s["layers"], 0.0, R)
    model.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()}, strict=True)
    return x, y, ei, et, model, ref


# ---- the restatement, pinned ------------------------------------------------------------------------------------------

def planted_run(aggr, act):
    """(out, g_rows, g_beta, g_gamma) of the planted graph on one channel under a cotangent of ones; the gradients
    [n, R]."""
    ei, n = graph_of("planted")
    et = edge_type_of("planted", PLANTED_R)
    rows, beta, gamma = (t.permute(1, 0, 2).clone().requires_grad_(True) for t in planted_tables(1))
    y0 = torch.tensor(PLANTED_Y0, dtype=torch.float64)[:, None]
    out = y0 + aggregate(rows, beta, gamma, n, ei[0], ei[1], et, aggr, act)
    out.sum().backward()
    return (out.detach().flatten(),) + tuple(t.grad[:, :, 0].t() for t in (rows, beta, gamma))


def test_restatement_reproduces_hand_computed_numbers():
    """h[j, r] = (0.5, 1, 1.5, 2, 2.5, 3)[j] + r; edges and relations of tests/test_rgcn_host.py's planted graph.
    target 0, three in-edges of relation 0 from 1, 2, 3 with gamma = -1 (the sign flips), beta = 1.75:
      z = 0.75, 0.25, -0.25 (one z < 0); relu: (0.75 + 0.25 + 0) / 3 = 1 / 3; identity: 0.75 / 3 = 0.25.
    target 1: relation 0 from node 0, gamma = 2, h = 0.5, beta = -1: z = 0 EXACTLY (the tie); relation 1 from node 2,
      1 * 2.5 + 0.5 = 3; relation 2 from node 3, 0.5 * 4 - 3 = -1. relu: 3; identity: 2.
    target 2: relation 1 twice from node 4 (duplicates of one type), 2 * 3.5 + 1 = 8 each: mean 8, sum 16; relation 0
      once from node 4, -2 * 2.5 + 6 = 1. mean: 9; add: 17.
    target 3: its self-loop of relation 2, 0.25 * 4 + 0 = 1. Nodes 4 and 5: no in-edge, out == y0. Relation 3 owns no
    edge; (target 0, relation 1) is a pair without an edge. y0 = 10, 20, .., 60."""
    third = 1.0 / 3.0
    out, g_rows, g_beta, g_gamma = planted_run("mean", "relu")
    assert torch.allclose(out, torch.tensor([10 + third, 23, 39, 41, 50, 60], dtype=torch.float64), rtol=0, atol=1e-12)
    assert out[4].item() == 50.0 and out[5].item() == 60.0                 # no in-edge: y0, bit for bit
    want = torch.zeros(6, PLANTED_R, dtype=torch.float64)
    want[1, 0], want[2, 0] = -third, -third                                # w = 1 / 3, gamma = -1, z > 0
    want[2, 1], want[3, 2] = 1.0, 0.25                                     # (3 -> 1 has z < 0: only the self-loop counts)
    want[4, 1], want[4, 0] = 2.0, -2.0                                     # two duplicates of weight 1 / 2 and gamma 2
    assert torch.allclose(g_rows, want, rtol=0, atol=1e-12)
    assert g_rows[0, 0].item() == 0.0 and g_rows[3, 0].item() == 0.0       # the tie and the z < 0: exact zeros
    wb, wg = torch.zeros(6, PLANTED_R, dtype=torch.float64), torch.zeros(6, PLANTED_R, dtype=torch.float64)
    wb[0, 0], wg[0, 0] = 2 * third, 2.5 * third                            # (1 + 1 + 0) / 3; (1 + 1.5) / 3
    wb[1, 1], wg[1, 1] = 1.0, 2.5
    wb[2, 1], wg[2, 1] = 1.0, 3.5
    wb[2, 0], wg[2, 0] = 1.0, 2.5
    wb[3, 2], wg[3, 2] = 1.0, 4.0
    assert torch.allclose(g_beta, wb, rtol=0, atol=1e-12) and torch.allclose(g_gamma, wg, rtol=0, atol=1e-12)
    assert g_beta[1, 0].item() == 0.0 and g_gamma[1, 0].item() == 0.0      # relu'(0) = 0 at the tie
    assert g_beta[1, 2].item() == 0.0 and g_gamma[1, 2].item() == 0.0      # z < 0
    assert g_beta[:, 3].abs().max().item() == 0.0 and g_rows[:, 3].abs().max().item() == 0.0   # the relation without an edge
    assert g_beta[0, 1].item() == 0.0                                      # a (target, relation) pair without an edge
    out_add = planted_run("add", "relu")[0]
    assert out_add.tolist() == [11.0, 23.0, 47.0, 41.0, 50.0, 60.0]
    assert planted_run("sum", "relu")[0].tolist() == out_add.tolist()
    out_id = planted_run("mean", None)[0]
    assert torch.allclose(out_id, torch.tensor([10.25, 22, 39, 41, 50, 60], dtype=torch.float64), rtol=0, atol=1e-12)
    assert planted_run("mean", "identity")[0].tolist() == out_id.tolist()
    et = edge_type_of("planted", PLANTED_R)
    assert int((et == PLANTED_R - 1).sum()) == 0 and int((graph_of("planted")[0][0] == graph_of("planted")[0][1]).sum()) == 1


def test_restatement_layer_follows_the_formula():
    """RefFiLMConv against the definition spelled out edge by edge in Python, beta FIRST in the split."""
    ei, n = graph_of("planted")
    et = edge_type_of("planted", PLANTED_R)
    x = f32_exact((n, 3), torch.Generator().manual_seed(1))
    for act in ("relu", None):
        ref = randomize(RefFiLMConv(3, 2, PLANTED_R, act=act), 2)
        f = (lambda t: t.clamp(min=0)) if act == "relu" else (lambda t: t)
        fs = ref.film_skip(x)
        want = f(fs[:, 2:] * ref.lin_skip(x) + fs[:, :2])
        for i in range(n):
            for r in range(PLANTED_R):
                into = [e for e in range(ei.size(1)) if int(ei[1, e]) == i and int(et[e]) == r]
                fr = ref.films[r](x[i])
                msgs = [f(fr[2:] * ref.lins[r](x[int(ei[0, e])]) + fr[:2]) for e in into]
                if into:
                    want[i] = want[i] + sum(msgs) / len(into)
        assert torch.allclose(ref(x, ei, et), want, rtol=0, atol=1e-12)


def test_beta_comes_first_in_the_split():
    """film = (beta | gamma): with the gamma half of every film zeroed the messages are act(beta) whatever h is; with the
    beta half zeroed and gamma one, they are act(h)."""
    ei, n = graph_of("n3")
    x = f32_exact((n, 3), torch.Generator().manual_seed(3))
    ref = randomize(RefFiLMConv(3, 2, 1), 4)
    with torch.no_grad():
        ref.films[0].weight[2:].zero_()
        ref.films[0].bias[2:].zero_()
    beta = ref.films[0](x)[:, :2]
    deg = torch.bincount(ei[1], minlength=n).double()[:, None]
    fs = ref.film_skip(x)
    skip = torch.relu(fs[:, 2:] * ref.lin_skip(x) + fs[:, :2])
    assert torch.allclose(ref(x, ei), skip + torch.relu(beta) * (deg > 0), rtol=0, atol=1e-12)
    rows, b, g = film_rows(torch.tensor([[1.0, 2.0]], dtype=torch.float64), torch.tensor([[3.0, 4.0, 5.0, 6.0]],
                                                                                         dtype=torch.float64), 1)
    assert b.flatten().tolist() == [3.0, 4.0] and g.flatten().tolist() == [5.0, 6.0] and rows.flatten().tolist() == [1.0, 2.0]


def test_restatement_sums_in_either_order():
    for graph, R in (("random", 3), ("planted", PLANTED_R)):
        case = operator_case(4, R, graph)
        a, b = run_formula(case, R, graph, "mean", "relu"), run_formula(case, R, graph, "mean", "relu", reverse=True)
        assert max(shares_of(b, a).values()) < 1e-6


def test_one_relation_is_the_formula_with_the_plain_mean():
    """R = 1: out_i = y0_i + mean over the in-edges of relu(gamma_i * h_j + beta_i)."""
    ei, n = graph_of("random")
    case = operator_case(4, 1, "random")
    h, fb, y0 = case[:3]
    z = fb[:, 4:][ei[1]] * h[ei[0]] + fb[:, :4][ei[1]]
    deg = torch.bincount(ei[1], minlength=n).clamp(min=1).double()
    want = y0 + torch.zeros(n, 4, dtype=torch.float64).index_add(0, ei[1], torch.relu(z)) / deg[:, None]
    assert torch.allclose(reference(4, 1, "random", "mean", "relu")[0], want, rtol=0, atol=1e-12)


def test_identity_is_a_bilinear_form():
    """act=None: out = y0 + A_r (gamma_r * (S h_r)) + cnt_r * beta_r, linear in h for fixed fb and in fb for fixed h;
    with aggr="add": sum_r gamma_r[i] * (sum of h_r over the in-edges of relation r) + #edges * beta_r[i]."""
    ei, n = graph_of("random")
    R, C = 3, 4
    et = edge_type_of("random", R)
    case = operator_case(C, R, "random")
    rows, beta, gamma = film_rows(case[0], case[1], R)
    want = case[2].clone()
    for r in range(R):
        s, d = ei[0][et == r], ei[1][et == r]
        hs = torch.zeros(n, C, dtype=torch.float64).index_add(0, d, rows[r][s])
        want = want + gamma[r] * hs + torch.bincount(d, minlength=n).double()[:, None] * beta[r]
    assert torch.allclose(run_formula(case, R, "random", "add", None)[0], want, rtol=0, atol=1e-9)


# ---- registry and module layout ----------------------------------------------------------------------------------------

def test_registry():
    from rgb_experiment_amd import nn as product_nn
    from rgb_experiment_amd.dist import experiment as dist_experiment
    from rgb_experiment_amd.initial_params import InitialParameters
    from rgb_experiment_amd.models import MODELS, REGISTRY
    assert MODELS["film"] is FiLM and "film" not in REGISTRY
    assert "film" not in dist_experiment.SUPPORTED
    assert "film" not in [str(m).lower() for m in InitialParameters().model_names]
    assert "FiLMConv" in product_nn.__all__ and product_nn.FiLMConv is FiLMConv
    assert list(inspect.signature(FiLM.__init__).parameters)[1:] == [
        "input_dim", "output_dim", "hidden_unit", "num_layers", "dropout_rate", "num_relations", "aggr"]
    assert inspect.signature(FiLM.__init__).parameters["num_relations"].default == 1
    assert list(inspect.signature(FiLM.forward).parameters)[1:] == ["x", "edge_index", "edge_type"]
    assert inspect.signature(FiLM.forward).parameters["edge_type"].default is None
    sig = inspect.signature(FiLMConv.__init__).parameters
    assert list(sig)[1:] == ["in_channels", "out_channels", "num_relations", "nn", "act", "aggr"]
    assert (sig["num_relations"].default, sig["nn"].default, sig["act"].default, sig["aggr"].default) == \
        (1, None, "relu", "mean")
    assert "3 * out" in FiLMConv.__doc__ and "unpinned" in FiLMConv.__doc__


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("custom", [False, True])
def test_parameter_names_shapes_and_strict_loading(custom, R):
    net = custom_net(7) if custom else None
    conv = FiLMConv(LAYER_F, 7, R, nn=net)
    want = {"lin_skip.weight": (7, LAYER_F)}
    for r in range(R):
        want[f"lins.{r}.weight"] = (7, LAYER_F)
    for key in [f"films.{r}" for r in range(R)] + ["film_skip"]:
        if custom:
            want.update({f"{key}.0.weight": (5, LAYER_F), f"{key}.0.bias": (5,), f"{key}.1.weight": (14, 5),
                         f"{key}.1.bias": (14,)})
        else:
            want[f"{key}.weight"] = (14, LAYER_F)
            if key != "film_skip":
                want[f"{key}.bias"] = (14,)                                # film_skip: Linear(in, 2 * out, bias=False)
    assert {k: tuple(v.shape) for k, v in conv.named_parameters()} == want
    assert sorted(conv.state_dict()) == sorted(want)
    if custom:                                                             # deep copies: no parameter is shared
        ids = [id(p) for p in conv.parameters()] + [id(p) for p in net.parameters()]
        assert len(set(ids)) == len(ids)
    ref = randomize(RefFiLMConv(LAYER_F, 7, R, net=net), 4)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    back = RefFiLMConv(LAYER_F, 7, R, net=net)
    back.load_state_dict({k: v.double() for k, v in conv.state_dict().items()}, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), ref.state_dict().values()))
    before = copy.deepcopy(conv.state_dict())
    torch.manual_seed(0)
    conv.reset_parameters()                                                # every parameter is redrawn
    assert all(not torch.equal(before[k], v) for k, v in conv.state_dict().items())


@pytest.mark.parametrize("R", MODEL_RELATIONS)
def test_model_layout(R):
    from rgb_experiment_amd.nn import BatchNorm1d
    x, y, ei, et, model, ref = model_case(R)
    s = MODEL_SHAPE
    assert len(model.convs) == s["layers"] and all(isinstance(c, FiLMConv) for c in model.convs)
    assert len(model.norms) == s["layers"] - 1 and all(isinstance(m, BatchNorm1d) for m in model.norms)
    assert [(c.in_channels, c.out_channels, c.act) for c in model.convs] == [(16, 12, "relu"), (12, 12, "relu"),
                                                                              (12, 5, None)]
    assert all(c.num_relations == R for c in model.convs)
    assert sorted(model.state_dict()) == sorted(ref.state_dict())
    back = copy.deepcopy(ref)
    back.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()},
                         strict=True)
    res = ref(x, ei, et)
    assert set(res) == {"out", "emb"} and res["out"].shape == (s["n"], s["classes"])
    with pytest.raises(ValueError, match="num_layers"):
        FiLM(4, 3, 8, 0, 0.5)
    assert len(FiLM(4, 3, 8, 1, 0.5).convs) == 1 and FiLM(4, 3, 8, 1, 0.5).convs[0].act is None


def test_kernel_channels_pads_what_the_layout_does_not_take():
    assert FiLMConv(4, 67).kernel_channels() == 68
    assert FiLMConv(4, 130).kernel_channels() == 132
    assert FiLMConv(4, 64).kernel_channels() == 64 and FiLMConv(4, 7).kernel_channels() == 7
    assert FiLMConv(4, 300).kernel_channels() == 300                       # blocks of 256 and 44
    assert FiLMConv(4, 323).kernel_channels() == 324                       # 256 and 67: padded to 68


def test_the_model_hands_edge_type_to_every_layer(monkeypatch):
    seen = []

    def forward(self, x, edge_index, edge_type=None):
        seen.append(edge_type)
        return x.new_zeros(x.size(0), self.out_channels) + x.mean()

    monkeypatch.setattr(FiLMConv, "forward", forward)
    x, y, ei, et, model, _ = model_case(4)
    model(x.float(), ei, et)
    assert len(seen) == MODEL_SHAPE["layers"] and all(s is et for s in seen)
    del seen[:]
    model(x.float(), ei)
    assert seen == [None] * MODEL_SHAPE["layers"]


# ---- refusals ------------------------------------------------------------------------------------------------------

HostGraph = RG.HostGraph


def test_layer_refusals():
    with pytest.raises(ValueError, match="in_channels"):
        FiLMConv((4, 4), 3)
    with pytest.raises(ValueError, match="in_channels"):
        FiLMConv(None, 3)
    for aggr in ("max", "min", "mul", None):
        with pytest.raises(ValueError, match="aggr"):
            FiLMConv(4, 3, aggr=aggr)
    for aggr in ("mean", "add", "sum"):
        FiLMConv(4, 3, aggr=aggr)
    for act in ("tanh", torch.tanh, nn.Tanh(), nn.Sigmoid(), F.relu, 1):
        with pytest.raises(NotImplementedError, match="act"):
            FiLMConv(4, 3, act=act)
    assert FiLMConv(4, 3, act=nn.ReLU()).act == "relu" and FiLMConv(4, 3).act == "relu"
    assert FiLMConv(4, 3, act=None).act is None and FiLMConv(4, 3, act="identity").act == "identity"
    with pytest.raises(ValueError):
        FiLMConv(4, 3, 0)
    conv = FiLMConv(4, 3, 2)
    x, ei, et = torch.randn(5, 4), torch.tensor([[0, 1, 2], [1, 2, 3]]), torch.tensor([0, 1, 0])
    with pytest.raises(ValueError, match="edge_type"):
        conv(x, ei)                                                        # required with num_relations > 1
    with pytest.raises(ValueError, match="edge_type"):
        conv(x, ei, et[:2])
    with pytest.raises(ValueError, match="edge_type"):
        conv(x, ei, et.to(torch.int32))
    with pytest.raises(ValueError, match="in_channels"):
        conv(torch.randn(5, 3), ei, et)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(x, ei, et)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FiLMConv(4, 3)(x, ei)                                              # one relation: no edge_type needed


def test_operator_refusals():
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, LOOPS_REMOVE_ADD

    class Partitioned:
        is_distributed = True
    et = torch.zeros(10, dtype=torch.int64)
    h, fb = torch.zeros(4, 8), torch.zeros(4, 16)
    with pytest.raises(RuntimeError, match="no node-partitioned form"):
        ops.film_aggregate(h, fb, Partitioned(), et, 2)
    graph = HostGraph(4, 10)
    with pytest.raises(ValueError, match="aggr"):
        ops.film_aggregate(h, fb, graph, et, 2, aggr="max")
    for act in ("tanh", torch.relu, 3):
        with pytest.raises(ValueError, match="act"):
            ops.film_aggregate(h, fb, graph, et, 2, act=act)
    for mode in (LOOPS_ADD_REMAINING, LOOPS_REMOVE_ADD):
        with pytest.raises(RuntimeError, match="LOOPS_KEEP"):
            ops.film_aggregate(h, fb, HostGraph(4, 10, loops_mode=mode), et, 2)
        with pytest.raises(RuntimeError, match="LOOPS_KEEP"):
            ops.film_aggregate(h, fb, HostGraph(4, 10, loops_mode=mode))
    with pytest.raises(ValueError, match="num_relations"):
        ops.film_aggregate(h, fb, graph, et, 0)
    with pytest.raises(ValueError, match="edge_type"):
        ops.film_aggregate(h, fb, graph, None, 2)                          # several relations need their vector
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.film_aggregate(torch.zeros(4, 7), fb, graph, et, 2)            # 7 columns are no 2 blocks
    with pytest.raises(RuntimeError, match="for a graph of"):
        ops.film_aggregate(torch.zeros(3, 8), fb, graph, et, 2)
    with pytest.raises(RuntimeError, match="fb"):
        ops.film_aggregate(h, torch.zeros(4, 8), graph, et, 2)             # fb holds 2C per relation
    with pytest.raises(RuntimeError, match="fb"):
        ops.film_aggregate(h, fb.double(), graph, et, 2)
    with pytest.raises(RuntimeError, match="y0"):
        ops.film_aggregate(h, fb, graph, et, 2, y0=torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.film_aggregate(h, fb, graph, et, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.film_aggregate(h, fb, graph)                                   # R = 1, no typed view: the device check
    for name in ("film_fwd_raw", "film_bwd_raw", "film_supported", "film_aggregate"):
        assert callable(getattr(ops, name))


def test_the_operand_range_beyond_int32_is_refused():
    """N * R >= 2^31 is refused before anything is launched or even moved: operands without storage suffice."""
    from rgb_experiment_amd import ops
    N, R = 2 ** 28, 8
    h = torch.empty((N, R), dtype=torch.float32, device="meta")
    fb = torch.empty((N, 2 * R), dtype=torch.float32, device="meta")
    with pytest.raises(RuntimeError, match="beyond int32"):
        ops.film_aggregate(h, fb, HostGraph(N, 10), torch.zeros(10, dtype=torch.int64), R)
    h7 = torch.empty((N, 7), dtype=torch.float32, device="meta")           # R = 7: N * R < 2^31, the device check is next
    fb7 = torch.empty((N, 14), dtype=torch.float32, device="meta")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.film_aggregate(h7, fb7, HostGraph(N, 10), torch.zeros(10, dtype=torch.int64), 7)


# ---- experiment(model_name="film") ---------------------------------------------------------------------------------------

FILM_INIT = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0, "num_relations": 3}
FILM_INIT_PLAIN = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0}


def test_experiment_refusals():
    run, data = G._run, RG._data
    film = dict(model_name="film", init=FILM_INIT, use_edge_type=True)
    for name in ("mlp", "gcn", "graphsage", "gat", "gine", "resgated"):
        with pytest.raises(ValueError, match="rgcn, film and a model="):
            run(data(True), model_name=name, use_edge_type=True)
    with pytest.raises(ValueError, match="to_undirected"):
        run(data(True), to_undirected_graph=True, **film)
    with pytest.raises(NotImplementedError, match="partitioned"):
        run(data(True), distributed=True, **film)
    with pytest.raises(NotImplementedError):
        run(data(True), print_pics=True, **film)
    with pytest.raises(ValueError, match="needs data.edge_type"):
        run(data(False), **film)
    with pytest.raises(ValueError, match="needs data.edge_type"):
        run(data(True, torch.zeros(300, dtype=torch.int32)), **film)
    with pytest.raises(ValueError, match=r"\[E\]"):
        run(data(True, torch.zeros(299, dtype=torch.int64)), **film)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # well-formed: the device check is next
        run(data(True), **film)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # and without edge types, with one relation
        run(data(False), model_name="film", init=FILM_INIT_PLAIN)
    with pytest.raises(ValueError, match="takes no edge attributes"):
        run(data(True), model_name="film", init=FILM_INIT, use_edge_attr=True)
    with pytest.raises(ValueError, match="takes no edge weights"):
        run(data(True), model_name="film", init=FILM_INIT, use_edge_weight=True)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

NEW_ENTRIES = ("rgbx_film_supported", "rgbx_film_fwd_f32", "rgbx_film_bwd_src_f32", "rgbx_film_bwd_film_f32")
loaded_lib = RG.loaded_lib


def test_abi_declares_and_exports_the_new_entries():
    from rgb_experiment_amd import _lib
    raw = open(os.path.join(ROOT, "include", "rgbx_hip.h")).read()
    assert "FiLMConv.forward [PyG]" in raw and "beta FIRST" in raw
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(rgbx_[a-z0-9_]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS, name
        params = re.search(name + r"\s*\(([^)]*)\)", text).group(1)       # one ctypes argument per declared parameter
        assert len(_lib.SIGNATURES[name]) == len([a for a in params.split(",") if a.strip()]), name
    assert loaded_lib().rgbx_version() == 501
    makefile = open(os.path.join(ROOT, "rgb_experiment_amd", "csrc", "Makefile")).read()
    assert "film.hip" in makefile


def test_film_supported_over_the_gpu_grid():
    lib = loaded_lib()
    for C in WIDTHS:
        assert lib.rgbx_film_supported(C), C
    for C in range(-1, 301):                                              # the widths of the shared lane layout, one head
        assert bool(lib.rgbx_film_supported(C)) == bool(lib.rgbx_transformer_supported(1, C)), C
    assert not lib.rgbx_film_supported(PADDED_WIDTH) and lib.rgbx_film_supported(PADDED_WIDTH + 1)
    assert not lib.rgbx_film_supported(0) and not lib.rgbx_film_supported(BLOCKED_WIDTH)
    assert lib.rgbx_film_supported(BLOCKED_WIDTH % 256) and lib.rgbx_film_supported(256)
    # vector widths as attn_common.h's pick_vec chooses them on aligned rows: all three occur in the grid
    assert {4 if C % 4 == 0 else (2 if C % 2 == 0 else 1) for C in WIDTHS} == {1, 2, 4}


def test_new_entries_validate_their_arguments():
    lib = loaded_lib()
    p = 0x10000  # 16-byte aligned, non-null, never dereferenced: every call below returns before a launch
    q = p + 0x100000

    def fwd(**kw):
        a = dict(rowptr=p, col=p, etype=p, w=p, h=p, ldh=64, fb=p, ldfb=128, gofs=64, y0=p, ldy=64, out=q, ldo=64, N=10,
                 R=3, C=64, mean=1, act=1)
        a.update(kw)
        return lib.rgbx_film_fwd_f32(a["rowptr"], a["col"], a["etype"], a["w"], a["h"], a["ldh"], a["fb"], a["ldfb"],
                                     a["gofs"], a["y0"], a["ldy"], a["out"], a["ldo"], a["N"], a["R"], a["C"], a["mean"],
                                     a["act"], None, None)
    for name in ("rowptr", "col", "h", "fb", "out", "w"):
        assert fwd(**{name: None}) == -1 and b"null" in lib.rgbx_last_error_string(), name
    assert fwd(etype=None) == -1 and b"single-relation" in lib.rgbx_last_error_string()   # R = 3 without types
    assert fwd(ldh=63) == -1 and b"leading dimension" in lib.rgbx_last_error_string()
    assert fwd(ldfb=127) == -1 and b"leading dimension" in lib.rgbx_last_error_string()
    assert fwd(gofs=63) == -1 and fwd(gofs=65) == -1 and fwd(ldo=63) == -1 and fwd(ldy=8) == -1
    for name in ("h", "fb", "y0"):
        assert fwd(out=p, **{name: p}) == -1 and b"alias" in lib.rgbx_last_error_string(), name
    assert fwd(R=0) == -1 and b"num_relations" in lib.rgbx_last_error_string()
    assert fwd(R=-2) == -1 and fwd(N=-1) == -1 and fwd(C=0) == -1
    assert fwd(act=2) == -1 and b"act" in lib.rgbx_last_error_string() and fwd(act=-1) == -1
    assert fwd(N=2 ** 31) == -2 and fwd(N=2 ** 30, R=3) == -2 and b"N * R" in lib.rgbx_last_error_string()
    assert fwd(C=67, ldh=67, ldfb=134, gofs=67, ldy=67, ldo=67) == -5                  # RGBX_E_SHAPE
    assert fwd(h=p + 2) == -3 and b"aligned" in lib.rgbx_last_error_string()
    assert fwd(fb=p + 1) == -3 and fwd(w=p + 3) == -3 and fwd(etype=p + 2) == -3 and fwd(y0=p + 2) == -3
    assert fwd(out=q + 2) == -3 and fwd(rowptr=p + 2) == -3 and fwd(col=p + 1) == -3
    # C = 256 needs 4 floats per lane: 16-byte pointers, leading dimensions and a gamma offset that are multiples of 4
    wide = dict(C=256, ldh=256, ldfb=512, gofs=256, ldy=256, ldo=256)
    assert fwd(**{**wide, "h": p + 8}) == -5 and b"lanes" in lib.rgbx_last_error_string()
    assert fwd(**{**wide, "ldh": 258}) == -5 and fwd(**{**wide, "gofs": 258, "ldfb": 516}) == -5
    assert fwd(N=0) == 0 and fwd(N=0, rowptr=None) == 0

    def src(**kw):
        a = dict(rowptr=p, col=p, w_t=p, deg=None, h=p, ldh=64, fb=p, ldfb=128, gofs=64, gout=p, ldg=64, g_h=q, ldgh=64,
                 N=1000, R=3, C=64, act=1)
        a.update(kw)
        return lib.rgbx_film_bwd_src_f32(a["rowptr"], a["col"], a["w_t"], a["deg"], a["h"], a["ldh"], a["fb"], a["ldfb"],
                                         a["gofs"], a["gout"], a["ldg"], a["g_h"], a["ldgh"], a["N"], a["R"], a["C"],
                                         a["act"], None, None)
    for name in ("rowptr", "col", "h", "fb", "gout", "g_h"):
        assert src(**{name: None}) == -1 and b"null" in lib.rgbx_last_error_string(), name
    assert src(ldh=63) == -1 and src(ldg=63) == -1 and src(ldgh=63) == -1 and src(ldfb=127) == -1 and src(gofs=32) == -1
    assert src(g_h=p) == -1 and b"alias" in lib.rgbx_last_error_string()
    assert src(R=0) == -1 and src(act=5) == -1
    assert src(gout=p + 2) == -3 and src(g_h=q + 1) == -3 and src(w_t=p + 2) == -3 and src(deg=p + 2) == -3
    assert src(C=130, ldh=130, ldg=130, ldgh=130, ldfb=260, gofs=130) == -5
    assert src(N=2 ** 31) == -2 and src(N=2 ** 29, R=4) == -2 and src(N=0) == 0

    def film(**kw):
        a = dict(rowptr=p, col=p, h=p, ldh=64, fb=p, ldfb=128, gofs=64, gout=p, ldg=64, g_fb=q, ldgfb=128, N=1000, R=3,
                 C=64, mean=1, act=1)
        a.update(kw)
        return lib.rgbx_film_bwd_film_f32(a["rowptr"], a["col"], a["h"], a["ldh"], a["fb"], a["ldfb"], a["gofs"], a["gout"],
                                          a["ldg"], a["g_fb"], a["ldgfb"], a["N"], a["R"], a["C"], a["mean"], a["act"],
                                          None, None)
    for name in ("rowptr", "col", "h", "fb", "gout", "g_fb"):
        assert film(**{name: None}) == -1 and b"null" in lib.rgbx_last_error_string(), name
    assert film(ldh=63) == -1 and film(ldg=32) == -1 and film(ldfb=100) == -1 and film(ldgfb=127) == -1
    assert film(gofs=200, ldfb=264) == -1                                 # g_fb keeps fb's layout: its rows are too short
    assert film(g_fb=p) == -1 and b"alias" in lib.rgbx_last_error_string()
    assert film(R=0) == -1 and film(act=2) == -1
    assert film(g_fb=q + 2) == -3 and film(h=p + 1) == -3
    assert film(C=67, ldh=67, ldg=67, ldfb=134, ldgfb=134, gofs=67) == -5
    assert film(N=2 ** 31) == -2 and film(N=2 ** 28, R=8) == -2 and film(N=0) == 0


# ---- preconditions of the GPU cases ----------------------------------------------------------------------------------

def expanded_lengths(name, R):
    """(in-edges per (target, relation), out-edges per (source, relation)), each int64 [n * R]: the row lengths of the
    two relation-expanded CSRs."""
    ei, n = graph_of(name)
    et = edge_type_of(name, R)
    return torch.bincount(ei[1] * R + et, minlength=n * R), torch.bincount(ei[0] * R + et, minlength=n * R)


def test_graphs_and_types_have_what_the_cases_need():
    from rgb_experiment_amd.graph import LONG_ROW_SLOTS as product_threshold
    assert LONG_ROW_SLOTS == product_threshold
    ei, n = graph_of("degrees")
    indeg, outdeg = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
    assert tuple(indeg[:6].tolist()) == G.DEGREES and tuple(outdeg[6:12].tolist()) == G.DEGREES
    for R in RELATIONS:   # rows of exactly 0 / 1 / 64 / 65 / T / T + 1 slots in both relation-expanded CSRs, one hub row each
        fin, fout = expanded_lengths("degrees", R)
        assert set(G.DEGREES) <= set(fin.tolist()) and set(G.DEGREES) <= set(fout.tolist())
        assert int((fin > LONG_ROW_SLOTS).sum()) == 1 and int((fout > LONG_ROW_SLOTS).sum()) == 1
        et = edge_type_of("degrees", R)
        assert int(et.min()) >= 0 and int(et.max()) <= max(R - 2, 0)        # the last relation owns no edge
        mixed = torch.bincount(ei[1] * R + et, minlength=n * R).view(n, R)[12:]
        assert R < 3 or int(((mixed > 0).sum(1) > 1).sum()) > 0           # targets that receive several relations
        fin, fout = expanded_lengths("powerlaw", R)
        print(f"powerlaw R = {R}: longest expanded forward row {int(fin.max())}, transposed {int(fout.max())}")
        # one relation keeps the hub rows of the plain CSRs (several spread them thin: `degrees` has the expanded hub
        # rows there); several relations leave (node, relation) rows without slots
        assert (int(fin.max()) > LONG_ROW_SLOTS and int(fout.max()) > LONG_ROW_SLOTS) if R == 1 else \
            (int(fin.min()) == 0 and int(fout.min()) == 0)
    cases = {(C, R, g) for C, R, g, _, _ in CASES}
    assert {(C, R) for C, R, g in cases if g == "degrees"} >= {(C, R) for C in WIDTHS for R in RELATIONS}
    for g in ("degrees", "powerlaw"):
        assert {4 if C % 4 == 0 else (2 if C % 2 == 0 else 1) for C, _, gg in cases if gg == g} == {1, 2, 4}
        assert {R for _, R, gg in cases if gg == g} == set(RELATIONS)
    assert {(aggr, act) for _, _, _, aggr, act in CASES} == {(a, b) for a in ("mean", "add") for b in ("relu", "identity")}
    assert {g for _, _, g in cases} >= set(graph_names) | {"planted"}


@pytest.mark.parametrize("C,R,graph,aggr,act", CASES)
def test_operator_case_is_well_posed(C, R, graph, aggr, act):
    case = operator_case(C, R, graph)
    assert all(torch.equal(t * 8, (t * 8).round()) and float(t.abs().max()) <= 60 for t in case[:4] if t.numel())
    ties = check_masks_agree(case, R, graph)
    ei, n = graph_of(graph)
    assert ties >= (len(range(0, ei.size(1), TIE_EVERY)) if graph != "planted" else C)
    want = reference(C, R, graph, aggr, act)
    low = run_formula(case, R, graph, aggr, act, dtype=torch.float32, reverse=True)
    shares = shares_of(low, want)
    print(f"C = {C} R = {R} {graph} {aggr} {act}: {ties} ties, max |out| {want[0].abs().max().item():.1f}; float32 "
          f"(reversed order) vs float64 share of tolerance {shares}")
    assert all(torch.isfinite(t).all() for t in [low[0]] + low[1])
    assert max(shares.values()) < WELL_POSED_SHARE, shares
    assert torch.equal(want[1][2], case[3])                               # g_y0 is the cotangent
    if graph == "no_edges":
        assert torch.equal(want[0], case[2]) and want[1][0].abs().max().item() == 0.0 and \
            want[1][1].abs().max().item() == 0.0
    if graph == "random":                                                 # rows without in-edges: out == y0
        assert torch.equal(want[0][:20], case[2][:20])
    if graph == "planted" and act == "relu":                              # the tie's gradient entries are exact zeros
        gh, gfb = want[1][0].view(6, PLANTED_R, C), want[1][1].view(6, PLANTED_R, 2 * C)
        assert gh[0, 0].abs().max().item() == 0.0 and gfb[1, 0].abs().max().item() == 0.0
        assert torch.equal(want[0][4:], case[2][4:])
    if R > 1 and graph != "planted":                                      # the relation without an edge
        assert want[1][0].view(n, R, C)[:, R - 1].abs().max().item() == 0.0
        assert want[1][1].view(n, R, 2 * C)[:, R - 1].abs().max().item() == 0.0


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
    return shares, low


def check_margins(ref, low, x, ei, et, x_err, what):
    margins = relu_margins(ref, x, ei, et, x_err)
    assert len(margins) == len(ref.relu_inputs) == len(low.relu_inputs)
    for k, ((z, margin), z64, z32) in enumerate(zip(margins, ref.relu_inputs, low.relu_inputs)):
        assert torch.equal(z, z64)
        if z.numel() == 0:
            continue
        print(f"{what} part {k}: min |relu input| {z.abs().min().item():.3e}, largest margin {margin.max().item():.3e}, "
              f"smallest |relu input| / margin {(z.abs() / margin).min().item():.1f}")
        assert bool((z.abs() > margin).all()), f"{what} part {k}: a relu input lies within float32's reach of zero"
        assert torch.equal(z32 > 0, z64 > 0)


@pytest.mark.parametrize("name", sorted(LAYER_CASES))
def test_layer_case_is_well_posed(name):
    x, ei, et, ref = layer_case(name)
    shares, low = module_shares(ref, lambda m, dt, rev: m(x.to(dt), ei, et, rev), 17)
    if ref.act == "relu":
        check_margins(ref, low, x, ei, et, 0.0, name)
    assert max(shares.values()) < WELL_POSED_SHARE, shares
    assert int((torch.bincount(ei[1], minlength=LAYER_N) == 0).sum()) > 0   # nodes without in-edges
    product_layer(name, ref)                                               # the product's layer takes the parameters


@pytest.mark.parametrize("R", MODEL_RELATIONS)
def test_model_case_is_well_posed(R):
    """The input of a conv behind the first is itself the output of float32 layers and arrives with an error, bounded
    from the reference alone as in tests/test_gine_host.model_margins: four times the deviation of the float32 reference
    run from the float64 one, plus BatchNorm's own rounding 3 u (|h| + |bias|)."""
    x, y, ei, et, model, ref = model_case(R)
    ref.train()
    shares, low = module_shares(ref, lambda m, dt, rev: m(x.to(dt), ei, et, rev)["out"], 18)
    for k, conv in enumerate(ref.convs):
        if conv.act != "relu":
            continue
        h64, h32 = ref.conv_inputs[k], low.conv_inputs[k].double()
        x_err = 0.0
        if k > 0:
            x_err = 4 * (h32 - h64).abs().max().item() + 3 * U32 * (h64.abs() + ref.norms[k - 1].bias.detach().abs())
        check_margins(conv, low.convs[k], h64, ei, et, x_err, f"conv {k}")
    assert max(shares.values()) < WELL_POSED_SHARE, shares
