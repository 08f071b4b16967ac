"""PNAConv on the host: a float64 restatement of the operator (u_p = b_j + c_p per edge, the six statistics of u over
the in-edges AS GIVEN, the shift by a, the five degree scalers, PyG's tower / scaler / aggregator column order) and of the
layer with PyG's dataflow (cat, per-tower pre_nn, aggregate, scale, cat, post_nn, lin), pinned by numbers derived by hand;
the layer's split of the message into a / b / c against that dataflow; registry, PyG's state_dict layout, refusals, the
use_edge_attr keyword of experiment() and the C ABI of the new entry points; and the case builders
tests/test_gpu_pna.py feeds to the HIP kernels, with the checks that keep those cases well-posed. No GPU needed.

Well-posedness. max / min pick a slot and std has a floor: a float32 run that picks another slot, or lands on the other
side of the floor, changes a whole gradient entry, which no tolerance covers. Every operator case therefore asserts, in
float64, that (1) the best u_p of every (row, channel) leads the best of the OTHER slots by >= 1e-5 * max(1, |u|) — a slot
with the winner's source and the winner's c value is the same float32 number as the winner, not an "other" slot: there
the lowest slot wins on both sides — except in the planted constant neighbourhoods, and (2) every variance is either
< 1e-9 (degree <= 1, duplicates, planted constant neighbourhoods) or > 1e-3. Random draws violate both somewhere among
10^5 (row, channel) pairs, whatever the seed; the builders REPAIR the draw (they move the c value — or, without c, the b
value — behind a violation by an order-1 amount and look again) until nothing is left, and the test asserts the
conditions on the result with no exclusions."""
import functools
import inspect
import math
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F_

from rgb_experiment_amd.models import PNA              # without the feature this file fails here, at import
from rgb_experiment_amd.nn import PNAConv

import test_gine_host as G
import test_transformer_host as T
from test_transformer_host import FWD_TOL, GRAD_TOL, f32_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AGGREGATORS = ("sum", "mean", "var", "std", "max", "min")
SCALERS = ("identity", "amplification", "attenuation", "linear", "inverse_linear")
DEFAULT_AGGR = ("mean", "max", "min", "std")
DEFAULT_SCALERS = ("identity", "amplification", "attenuation")
STD_FLOOR = 1e-5


# ---- the restatement ---------------------------------------------------------------------------------------------------

def scale_factors(deg, scalers, avg):
    """[n, S]: scale_s of every node, D = max(deg, 1), avg = (avg_lin, avg_log)."""
    D = deg.clamp(min=1).double()
    logD = torch.log(D + 1)
    lin, log = float(avg[0]), float(avg[1])
    cols = {"identity": torch.ones_like(D), "amplification": logD / log, "attenuation": log / logD, "linear": D / lin,
            "inverse_linear": lin / D}
    return torch.stack([cols[s] for s in scalers], dim=1)


def aggregate_scale(u, a, n, dst, aggregators, scalers, avg, F):
    """out [n, T*S*A*F] from the messages u [E, d] (one row per edge, in the order of the edge list) and the target part
    a [n, d] (or None), in the precision of the inputs; info: the raw var and the winning slots (forward CSR numbering:
    the edges stably grouped by target). Every statistic written from its definition; the extrema gather the value of
    the LOWEST slot that attains them, so autograd sends their whole gradient there."""
    E, d = u.shape
    order = torch.argsort(dst, stable=True)
    us, ds = u[order], dst[order]
    deg = torch.bincount(dst, minlength=n)
    has = (deg > 0)[:, None]
    D = deg.clamp(min=1).to(u.dtype)[:, None]
    zeros = torch.zeros(n, d, dtype=u.dtype)
    total = zeros.index_add(0, ds, us)
    mean = total / D
    var = zeros.index_add(0, ds, (us - mean[ds]) ** 2) / D
    std = torch.where(var > STD_FLOOR, var.clamp(min=STD_FLOOR).sqrt(), zeros)
    idx = ds[:, None].expand(E, d)
    slot = torch.arange(E)[:, None].expand(E, d)

    def extremum(sign):
        if E == 0:
            return zeros, torch.full((n, d), -1, dtype=torch.int64)
        v = (sign * us).detach()
        best = torch.full((n, d), -math.inf, dtype=u.dtype).scatter_reduce(0, idx, v, "amax")
        cand = torch.where(v == best[ds], slot, torch.full_like(slot, E))
        arg = torch.full((n, d), E, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin")
        val = torch.where(has, us.gather(0, arg.clamp(max=E - 1)), zeros)
        return val, torch.where(has, arg, torch.full_like(arg, -1))

    mx, argmax = extremum(1.0)
    mn, argmin = extremum(-1.0)
    if a is not None:   # a row without slots stays 0: no message, nothing to shift
        total = total + deg.to(u.dtype)[:, None] * a
        mean, mx, mn = mean + a * has, mx + a * has, mn + a * has
    stat = {"sum": total, "mean": mean, "var": var, "std": std, "max": mx, "min": mn}
    fac = scale_factors(deg, scalers, avg).to(u.dtype)
    Tn = d // F
    out = torch.stack([torch.stack([fac[:, s, None, None] * stat[k].view(n, Tn, F) for k in aggregators], dim=2)
                       for s in range(len(scalers))], dim=2)                       # [n, T, S, A, F]
    return out.reshape(n, -1), {"var": var.detach(), "argmax": argmax, "argmin": argmin, "deg": deg}


def operator(a, b, c, n, src, dst, aggregators, scalers, avg, F):
    """The operator of the layer's contract: u_p = b[src] + c (c [E, d] in the order of the edge list, or None)."""
    u = b.index_select(0, src)
    return aggregate_scale(u if c is None else u + c, a, n, dst, aggregators, scalers, avg, F)


class RefPNAConv(nn.Module):
    """float64 restatement of PNAConv with PyG's dataflow and PyG's parameter names. `avg` = (avg_lin, avg_log)."""

    def __init__(self, in_channels, out_channels, aggregators, scalers, avg, edge_dim=None, towers=1, post_layers=1,
                 divide_input=False):
        super().__init__()
        self.aggregators, self.scalers, self.avg = tuple(aggregators), tuple(scalers), avg
        self.towers, self.divide_input, self.edge_dim = towers, divide_input, edge_dim
        self.F_in = in_channels // towers if divide_input else in_channels
        self.F_out = out_channels // towers
        if edge_dim is not None:
            self.edge_encoder = nn.Linear(edge_dim, self.F_in)
        self.pre_nns, self.post_nns = nn.ModuleList(), nn.ModuleList()
        for _ in range(towers):
            self.pre_nns.append(nn.Sequential(nn.Linear((3 if edge_dim is not None else 2) * self.F_in, self.F_in)))
            post = [nn.Linear((len(aggregators) * len(scalers) + 1) * self.F_in, self.F_out)]
            for _ in range(post_layers - 1):
                post += [nn.ReLU(), nn.Linear(self.F_out, self.F_out)]
            self.post_nns.append(nn.Sequential(*post))
        self.lin = nn.Linear(out_channels, out_channels)
        self.double()
        self.messages = None

    def forward(self, x, ei, ea=None):
        src, dst = ei[0], ei[1]
        n, Tn, Fi = x.size(0), self.towers, self.F_in
        xt = x.view(n, Tn, Fi) if self.divide_input else x.view(n, 1, Fi).repeat(1, Tn, 1)
        parts = [xt[dst], xt[src]]
        if self.edge_dim is not None:
            parts.append(self.edge_encoder(ea).view(-1, 1, Fi).repeat(1, Tn, 1))
        h = torch.cat(parts, dim=-1)
        m = torch.stack([pre(h[:, t]) for t, pre in enumerate(self.pre_nns)], dim=1).reshape(-1, Tn * Fi)
        self.messages = m.detach()
        agg, _ = aggregate_scale(m, None, n, dst, self.aggregators, self.scalers, self.avg, Fi)
        out = torch.cat([xt, agg.view(n, Tn, -1)], dim=-1)
        out = torch.cat([post(out[:, t]) for t, post in enumerate(self.post_nns)], dim=1)
        return self.lin(out)


class RefPNA(nn.Module):
    """models/pna.py in float64; the product's module names."""

    def __init__(self, input_dim, output_dim, hidden_unit, num_layers, dropout_rate, avg, aggregators=DEFAULT_AGGR,
                 scalers=DEFAULT_SCALERS, towers=1, edge_dim=None, post_layers=1):
        super().__init__()
        dims = [input_dim] + [hidden_unit] * (num_layers - 1) + [output_dim]
        self.convs = nn.ModuleList(
            RefPNAConv(a, b, aggregators, scalers, avg, edge_dim, towers if i + 2 < len(dims) else 1, post_layers)
            for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])))

    def forward(self, x, ei, ea=None):
        for i, conv in enumerate(self.convs):
            x = conv(x, ei, ea)
            if i + 1 < len(self.convs):
                x = F_.relu(x)
        return {"out": F_.log_softmax(x, dim=1), "emb": x}


def averages_of(ei, n):
    """(avg_lin, avg_log) of a graph's in-degrees as float32 values: PyG's histogram form."""
    hist = torch.bincount(torch.bincount(ei[1], minlength=n)).double()
    bins = torch.arange(hist.numel(), dtype=torch.float64)
    avg = torch.stack([(bins * hist).sum(), ((bins + 1).log() * hist).sum()]) / hist.sum()
    return avg.float()


# ---- operator cases shared with tests/test_gpu_pna.py ----------------------------------------------------------------

graph_of, slots_of = G.graph_of, G.slots_of
WIDTHS = [4, 8, 32, 64, 128, 256]
TOWER_SPLITS = [(8, 4), (64, 16), (256, 64)]
BLOCKED = (320, 64)
FIXED_AVG = torch.tensor([2.5, 1.25])      # graphs whose own averages are 0 (PyG itself produces NaN there)
OWN_AVG_GRAPHS = ("random", "powerlaw", "degrees")
N_TIES = 4


def avg_of(graph_name):
    ei, n = graph_of(graph_name)
    return averages_of(ei, n) if graph_name in OWN_AVG_GRAPHS else FIXED_AVG


@functools.lru_cache(maxsize=None)
def planted(graph_name):
    """(tie pairs [(p, q)] of edge ids: duplicate edges, each pair into a row of its own; constant row or None)."""
    ei, n = graph_of(graph_name)
    if graph_name not in ("random", "powerlaw"):
        return (), None
    key = (ei[0] * n + ei[1]).tolist()
    first, pairs, rows = {}, [], set()
    for e, k in enumerate(key):
        if k in first and int(ei[1, e]) not in rows and len(pairs) < N_TIES:
            pairs.append((first[k], e))
            rows.add(int(ei[1, e]))
        first.setdefault(k, e)
    deg = torch.bincount(ei[1], minlength=n)
    const = next(r for r in range(n) if 3 <= int(deg[r]) <= 12 and r not in rows)
    return tuple(pairs), const


def violations(u, src, dst, n, skip_rows=(), detail=None):
    """(gap violations, var violations): boolean [n, d] each, from the float64 messages u [E, d] in edge order.
    `detail` (a dict) receives, per sign (+1 the max, -1 the min), (violations [n, d], winning edge ids [n, d])."""
    E, d = u.shape
    zeros = torch.zeros(n, d, dtype=torch.float64)
    if E == 0:
        return zeros.bool(), zeros.bool()
    deg = torch.bincount(dst, minlength=n)
    D = deg.clamp(min=1).double()[:, None]
    mean = zeros.index_add(0, dst, u) / D
    var = zeros.index_add(0, dst, (u - mean[dst]) ** 2) / D
    bad_var = (var >= 1e-9) & (var <= 1e-3)
    idx = dst[:, None].expand(E, d)
    bad_gap = zeros.bool()
    eid = torch.arange(E)[:, None].expand(E, d)
    for sign in (1.0, -1.0):
        v = sign * u
        best = torch.full((n, d), -math.inf, dtype=torch.float64).scatter_reduce(0, idx, v, "amax")
        win = torch.full((n, d), E, dtype=torch.int64).scatter_reduce(0, idx, torch.where(v == best[dst], eid, E), "amin")
        wsrc = src[win.clamp(max=E - 1)]                                   # [n, d] source of the winning edge
        same = (v == best[dst]) & (src[:, None] == wsrc[dst])                  # the winner and its exact copies
        rest = torch.full((n, d), -math.inf, dtype=torch.float64).scatter_reduce(
            0, idx, torch.where(same, torch.full_like(v, -math.inf), v), "amax")
        bad = (deg > 0)[:, None] & (best - rest < 1e-5 * best.abs().clamp(min=1))
        for r in skip_rows:
            bad[r] = False
        if detail is not None:
            detail[sign] = (bad, win)
        bad_gap |= bad
    return bad_gap, bad_var


@functools.lru_cache(maxsize=8)
def operator_case(d, graph_name, with_c=True, offset=0.0):
    """a, b [n, d], c [E, d] in edge order (None without c), the cotangent seed: float64, fp32-exact, N(0, 1); planted
    ties and a planted constant neighbourhood on `random` / `powerlaw`; repaired until well-posed (module docstring)."""
    ei, n = graph_of(graph_name)
    src, dst = ei[0], ei[1]
    E = ei.size(1)
    g = torch.Generator().manual_seed(7000 + d + (0 if with_c else 500))
    a, b = f32_exact((n, d), g), f32_exact((n, d), g)
    c = f32_exact((E, d), g) if with_c else None
    if offset:
        b = (b + offset).float().double()
    pairs, const = planted(graph_name)
    if with_c:
        for p, q in pairs:          # identical c rows on a duplicate edge: an exact tie, the max of channel 0, the min of 1
            c[p, 0], c[p, 1] = 40.0, -40.0
            c[q] = c[p]
        if const is not None:       # u_p = 3 in every slot and channel, exactly, in float32 and in float64
            rows = (dst == const).nonzero(as_tuple=True)[0]
            b[src[rows]] = torch.round(b[src[rows]] * 64) / 64
            c[rows] = 3.0 - b[src[rows]]
    skip = (const,) if (with_c and const is not None) else ()
    frozen = torch.zeros(E, dtype=torch.bool)
    if with_c:
        for p, q in pairs:
            frozen[p] = frozen[q] = True
        if const is not None:
            frozen[dst == const] = True
    def move(e, ch, step):
        if c is not None:
            c[e, ch] = (c[e, ch] + step).float().double()
        else:
            b[src[e], ch] = (b[src[e], ch] + step).float().double()

    for _ in range(60):
        u = b[src] if c is None else b[src] + c
        detail = {}
        bad_gap, bad_var = violations(u, src, dst, n, skip, detail)
        if not bool((bad_gap | bad_var).any()):
            break
        for sign, (bad, win) in detail.items():            # a near-tie: the winner moves further out
            for r, ch in bad.nonzero().tolist():
                move(int(win[r, ch]), ch, sign * float(torch.round((1.0 + torch.rand(1, generator=g)) * 16) / 16))
        for r, ch in bad_var.nonzero().tolist():            # a variance in the band: one value of the row moves
            edges = ((dst == r) & ~frozen).nonzero(as_tuple=True)[0]
            if edges.numel():
                e = int(edges[int(torch.randint(0, edges.numel(), (1,), generator=g))])
                move(e, ch, float(torch.round((1.0 + torch.rand(1, generator=g)) * 16) / 16) * (1 if r % 2 else -1))
    return a, b, c


def cotangent(n, width, seed):
    return f32_exact((n, width), torch.Generator().manual_seed(seed))


def run_formula(case, graph_name, aggregators, scalers, F, with_a=True):
    """(out, [g_a, g_b, g_c], info) of a case in float64; g_c in the order of the edge list (None without c)."""
    ei, n = graph_of(graph_name)
    a, b, c = (None if t is None else t.clone().requires_grad_(True) for t in case)
    if not with_a:
        a = None
    out, info = operator(a, b, c, n, ei[0], ei[1], aggregators, scalers, avg_of(graph_name), F)
    cot = cotangent(n, out.size(1), 99)
    (out * cot).sum().backward()
    return out.detach(), [None if t is None else t.grad for t in (a, b, c)], info


@functools.lru_cache(maxsize=4)
def reference(d, F, graph_name):
    """The float64 result of a main case (default 4 x 3), computed once and shared (read-only)."""
    return run_formula(operator_case(d, graph_name), graph_name, DEFAULT_AGGR, DEFAULT_SCALERS, F)


OPERATOR_CASES = ([(d, d, g) for d in WIDTHS for g in T.GRAPH_NAMES] + [(32, 32, "degrees"), (256, 256, "degrees")]
                  + [(d, d, g) for d in (4, 64) for g in G.SMALL_GRAPHS]
                  + [(d, F, "random") for d, F in TOWER_SPLITS] + [(64, 16, "powerlaw"), BLOCKED + ("random",)])
OPTION_CASE = (32, "random")


# ---- the restatement is pinned -------------------------------------------------------------------------------------------

def t64(rows):
    return torch.tensor(rows, dtype=torch.float64)


def test_restatement_by_hand():
    """Three nodes, one channel pair (d = 2, F = 2). Edges 0 -> 2 (c = (1, 0)), 1 -> 2 (c = (0, 2)), 0 -> 1 (c = (0, 0));
    b = (1, 2), (3, -1), (9, 9); a = (10, 20), (1, 1), (100, 200). Row 2: u = (2, 2), (3, 1): sum (5, 3), mean (5/2, 3/2),
    var (1/4, 1/4), std (1/2, 1/2), max (3, 2), min (2, 1), argmax slots (2, 1), argmin (1, 2) (slot 0 is row 1's edge).
    With a: sum + 2 a = (205, 403), mean (102.5, 201.5), max (103, 202), min (102, 201). Row 1: one slot u = (1, 2): var 0,
    std 0, everything else u + a = (2, 3). Row 0: no slot: zeros. avg = (1, log 2): amplification = log(D + 1) / log 2 =
    1 for D = 1 and log 3 / log 2 for D = 2; linear = D; inverse_linear = 1 / D."""
    b, a = t64([[1, 2], [3, -1], [9, 9]]), t64([[10, 20], [1, 1], [100, 200]])
    c = t64([[1, 0], [0, 2], [0, 0]])
    src, dst = torch.tensor([0, 1, 0]), torch.tensor([2, 2, 1])
    avg = (1.0, math.log(2.0))
    out, info = operator(a, b, c, 3, src, dst, AGGREGATORS, ("identity",), avg, 2)
    assert torch.equal(out[0], torch.zeros(12, dtype=torch.float64))
    assert torch.equal(out[1], t64([2, 3, 2, 3, 0, 0, 0, 0, 2, 3, 2, 3]))
    assert torch.equal(out[2], t64([205, 403, 102.5, 201.5, 0.25, 0.25, 0.5, 0.5, 103, 202, 102, 201]))
    assert info["argmax"].tolist() == [[-1, -1], [0, 0], [2, 1]] and info["argmin"].tolist() == [[-1, -1], [0, 0], [1, 2]]
    out, _ = operator(None, b, c, 3, src, dst, ("max",), SCALERS, avg, 2)
    amp = math.log(3.0) / math.log(2.0)
    assert torch.allclose(out[2], t64([3, 2, 3 * amp, 2 * amp, 3 / amp, 2 / amp, 6, 4, 1.5, 1]), rtol=0, atol=1e-14)
    assert torch.allclose(out[1], t64([1, 2] * 5), rtol=0, atol=1e-14) and torch.equal(out[0], torch.zeros(10, dtype=torch.float64))
    out, _ = operator(None, b, None, 3, src, dst, ("sum",), ("identity",), avg, 2)      # c absent: u = b[src]
    assert torch.equal(out, t64([[0, 0], [1, 2], [4, 1]]))


def test_restatement_towers_and_column_order():
    """d = 4 as T = 2 towers of F = 2: column t*S*A*F + (s*A + k)*F + f."""
    g = torch.Generator().manual_seed(1)
    b, c = f32_exact((4, 4), g), f32_exact((5, 4), g)
    src, dst = torch.tensor([0, 1, 2, 3, 0]), torch.tensor([1, 1, 1, 0, 0])
    avg = (1.5, 1.0)
    wide, _ = operator(None, b, c, 4, src, dst, ("mean", "max"), ("identity", "linear"), avg, 2)
    assert wide.shape == (4, 2 * 2 * 2 * 2)
    for t in range(2):
        one, _ = operator(None, b[:, 2 * t:2 * t + 2], c[:, 2 * t:2 * t + 2], 4, src, dst, ("mean", "max"),
                          ("identity", "linear"), avg, 2)
        assert torch.equal(wide[:, 8 * t:8 * t + 8], one)
    mean, _ = operator(None, b, c, 4, src, dst, ("mean",), ("identity",), avg, 4)
    assert torch.equal(wide[:, 0:2], mean[:, 0:2]) and torch.equal(wide[:, 8:10], mean[:, 2:4])
    assert torch.allclose(wide[1, 4:6], 3 / 1.5 * mean[1, 0:2]) and torch.allclose(wide[0, 12:14], 2 / 1.5 * mean[0, 2:4])


def test_restatement_tie_gradient_goes_to_the_lowest_slot():
    b = t64([[1.0, 5.0], [0.0, 0.0]]).requires_grad_(True)
    c = t64([[2.0, 0.0], [2.0, 0.0], [1.0, 0.0]]).requires_grad_(True)
    src, dst = torch.tensor([0, 0, 0]), torch.tensor([1, 1, 1])
    out, info = operator(None, b, c, 2, src, dst, ("max", "min"), ("identity",), (1.0, 1.0), 2)
    assert info["argmax"][1].tolist() == [0, 0] and info["argmin"][1].tolist() == [2, 0]
    out[1, 0].backward()
    assert c.grad.tolist() == [[1.0, 0.0], [0.0, 0.0], [0.0, 0.0]]


def test_degree_averages_match_the_histogram_form():
    from rgb_experiment_amd import ops
    for name in OWN_AVG_GRAPHS:
        ei, n = graph_of(name)
        host = G.HostGraph(name)
        host.fwd.rowptr = slots_of(name)[2].to(torch.int32)
        got = ops.degree_averages(host)
        assert got.dtype == torch.float32 and got.shape == (2,) and ops.degree_averages(host) is got
        assert torch.allclose(got, averages_of(ei, n), rtol=1e-6, atol=0)
        deg = torch.bincount(ei[1], minlength=n).double()
        assert abs(got[0].item() - deg.mean().item()) < 1e-5 * deg.mean().item()
    empty = G.HostGraph("no_edges")
    empty.fwd.rowptr = torch.zeros(graph_of("no_edges")[1] + 1, dtype=torch.int32)
    assert ops.degree_averages(empty).tolist() == [0.0, 0.0]


# ---- well-posedness of every case ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,F,graph", OPERATOR_CASES)
def test_operator_case_is_well_posed(d, F, graph):
    case = operator_case(d, graph)
    assert all(torch.equal(t, t.float().double()) for t in case)              # exactly representable in float32
    ei, n = graph_of(graph)
    pairs, const = planted(graph)
    u = case[1][ei[0]] + case[2]
    bad_gap, bad_var = violations(u, ei[0], ei[1], n, (const,) if const is not None else ())
    assert not bool(bad_gap.any()) and not bool(bad_var.any())
    if graph in ("random", "powerlaw"):
        assert len(pairs) == N_TIES and const is not None
        rows = (ei[1] == const).nonzero(as_tuple=True)[0]
        assert rows.numel() >= 3 and bool((u[rows] == 3.0).all())
        assert bool(((case[1].float()[ei[0][rows]] + case[2].float()[rows]) == 3.0).all())   # and in float32
        for p, q in pairs:
            assert ei[:, p].tolist() == ei[:, q].tolist() and torch.equal(case[2][p], case[2][q])
            r = int(ei[1, p])
            assert u[p, 0] == u[ei[1] == r][:, 0].max() and u[p, 1] == u[ei[1] == r][:, 1].min()
    avg = avg_of(graph)
    assert float(avg[0]) > 0 and float(avg[1]) > 0


def test_option_cases_are_well_posed():
    d, graph = OPTION_CASE
    ei, n = graph_of(graph)
    for with_c in (True, False):
        a, b, c = operator_case(d, graph, with_c)
        u = b[ei[0]] if c is None else b[ei[0]] + c
        const = planted(graph)[1] if with_c else None
        bad_gap, bad_var = violations(u, ei[0], ei[1], n, (const,) if const is not None else ())
        assert not bool(bad_gap.any()) and not bool(bad_var.any())
    a, b, c = operator_case(d, graph, False, 1000.0)                         # the offset case keeps its variances
    bad_gap, bad_var = violations(b[ei[0]], ei[0], ei[1], n)
    assert not bool(bad_gap.any()) and not bool(bad_var.any())
    out, _, info = run_formula((a, b, c), graph, ("var", "std"), ("identity",), d)
    _, _, plain = run_formula(operator_case(d, graph, False), graph, ("var", "std"), ("identity",), d)
    assert float(b.mean()) > 900 and 0.5 < float(info["var"].mean() / plain["var"].mean()) < 2.0
    assert float(out.abs().max()) < 100.0


# ---- layer and model cases ----------------------------------------------------------------------------------------------

LAYER_N = 90
LAYER_CONFIGS = [  # (in, out, towers, edge_dim, divide_input, post_layers)
    (8, 8, 1, None, False, 1), (8, 8, 1, 5, False, 2), (8, 12, 4, None, False, 1), (8, 12, 4, 5, False, 1),
    (16, 8, 4, 5, True, 1), (16, 8, 4, None, True, 2), (6, 8, 1, 5, False, 1), (24, 8, 4, None, True, 1)]
# F_in: 8, 8, 8, 8, 4, 4, 6 (padded to 8), 6 (padded to 8, four towers)


@functools.lru_cache(maxsize=None)
def layer_graph():
    """Nodes 0..4 without in-edges, 5..9 with one, the rest with six from random sources; four duplicate edges and four
    self-loops on top; shuffled."""
    g = torch.Generator().manual_seed(8800)
    src, dst = [], []
    for i in range(5, LAYER_N):
        k = 1 if i < 10 else 6
        src.append(torch.randint(0, LAYER_N, (k,), generator=g))
        dst.append(torch.full((k,), i))
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    loops = torch.arange(20, 24)
    ei = torch.cat([ei, ei[:, 100:104], torch.stack([loops, loops])], dim=1)
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()


def layer_case(config, seed=0):
    """(x, edge_index, edge_attr or None, reference layer with fp32-exact parameters, averages)."""
    cin, cout, towers, edge_dim, divide, post_layers = config
    ei = layer_graph()
    g = torch.Generator().manual_seed(8900 + 13 * cin + cout + towers + seed)
    x = f32_exact((LAYER_N, cin), g)
    ea = f32_exact((ei.size(1), edge_dim), g) if edge_dim is not None else None
    avg = averages_of(ei, LAYER_N)
    ref = RefPNAConv(cin, cout, DEFAULT_AGGR, DEFAULT_SCALERS, avg, edge_dim, towers, post_layers, divide)
    with torch.no_grad():
        for key, prm in ref.named_parameters():
            prm.copy_(f32_exact(prm.shape, g, prm.size(-1) ** -0.5 if key.endswith("weight") else 0.5))
    return x, ei, ea, ref, avg


def product_layer(ref, config, deg=None):
    cin, cout, towers, edge_dim, divide, post_layers = config
    conv = PNAConv(cin, cout, list(DEFAULT_AGGR), list(DEFAULT_SCALERS), deg=deg, edge_dim=edge_dim, towers=towers,
                   post_layers=post_layers, divide_input=divide)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return conv


@pytest.mark.parametrize("config", LAYER_CONFIGS)
def test_layer_split_equals_the_pyg_dataflow(config):
    """a | b from the layer's one GEMM, c from its folded edge GEMM, the operator, then the post-networks on the
    unpadded blocks: the float64 restatement of PyG's cat -> pre_nn -> aggregate -> scale -> cat -> post_nn -> lin."""
    x, ei, ea, ref, avg = layer_case(config)
    want = ref(x, ei, ea)
    bad_gap, bad_var = violations(ref.messages, ei[0], ei[1], LAYER_N)
    assert not bool(bad_gap.any()) and not bool(bad_var.any()), "layer case is not well-posed: take the next seed"
    conv = product_layer(ref, config).double()
    Fi, Tn = conv.F_in, conv.towers
    Fp = (Fi + 3) // 4 * 4
    w, bias = conv._node_operands()
    ab = x @ w.t() + bias
    c = None
    if ea is not None:
        wc, bc = conv._edge_operands()
        assert wc.shape == (Tn * Fp, config[3])                                # ONE product at the raw edge width
        c = ea @ wc.t() + bc
    assert ab.shape == (LAYER_N, 2 * Tn * Fp)
    agg, _ = operator(ab[:, :Tn * Fp], ab[:, Tn * Fp:], c, LAYER_N, ei[0], ei[1], DEFAULT_AGGR, DEFAULT_SCALERS, avg, Fp)
    blocks = len(DEFAULT_AGGR) * len(DEFAULT_SCALERS)
    agg = agg.view(LAYER_N, Tn, blocks, Fp)[..., :Fi].reshape(LAYER_N, Tn, blocks * Fi)
    if Fp != Fi:
        assert float(ab.detach().view(LAYER_N, 2 * Tn, Fp)[..., Fi:].abs().max()) == 0.0   # padded channels carry zeros
    xt = x.view(LAYER_N, Tn, Fi) if config[4] else x.view(LAYER_N, 1, Fi).repeat(1, Tn, 1)
    out = torch.cat([post(torch.cat([xt[:, t], agg[:, t]], dim=-1)) for t, post in enumerate(conv.post_nns)], dim=1)
    got = conv.lin(out)
    assert (got - want).abs().max().item() < 1e-10 * max(1.0, want.abs().max().item())


MODEL_SHAPE = dict(f=8, hidden=8, classes=5, layers=3, towers=2, edge_dim=5)


MODEL_SEEDS = {False: 9500, True: 9500}     # the first seeds whose reference run is well-posed (asserted below)


def model_case(with_edges):
    """(x, y, edge_index, edge_attr, the product's model on the CPU, the reference holding its parameters)."""
    s = MODEL_SHAPE
    ei = layer_graph()
    g = torch.Generator().manual_seed(MODEL_SEEDS[with_edges])
    x = f32_exact((LAYER_N, s["f"]), g)
    ea = f32_exact((ei.size(1), s["edge_dim"]), g) if with_edges else None
    y = torch.randint(0, s["classes"], (LAYER_N,), generator=g)
    torch.manual_seed(9500)
    kw = dict(towers=s["towers"], edge_dim=s["edge_dim"] if with_edges else None)
    model = PNA(s["f"], s["classes"], s["hidden"], s["layers"], 0.0, **kw)
    with torch.no_grad():   # order-1 messages in every layer (the default init shrinks them layer by layer), biases off zero
        for key, prm in model.named_parameters():
            prm.copy_(torch.randn(prm.shape, generator=g) * (1.5 * prm.size(-1) ** -0.5 if key.endswith("weight") else 0.3))
    ref = RefPNA(s["f"], s["classes"], s["hidden"], s["layers"], 0.0, averages_of(ei, LAYER_N), **kw)
    ref.load_state_dict({k: v.double() for k, v in model.state_dict().items()}, strict=True)
    return x, y, ei, ea, model, ref


@pytest.mark.parametrize("with_edges", [False, True])
def test_model_case_is_well_posed(with_edges):
    x, y, ei, ea, model, ref = model_case(with_edges)
    res = ref(x, ei, ea)
    assert set(res) == {"out", "emb"} and res["out"].shape == (LAYER_N, MODEL_SHAPE["classes"])
    for conv in ref.convs:
        bad_gap, bad_var = violations(conv.messages, ei[0], ei[1], LAYER_N)
        assert not bool(bad_gap.any()) and not bool(bad_var.any())


# ---- registry, module layout, refusals -----------------------------------------------------------------------------------

def test_registry():
    from rgb_experiment_amd.dist import experiment as dist_experiment
    from rgb_experiment_amd.initial_params import InitialParameters
    from rgb_experiment_amd.models import MODELS, REGISTRY
    from rgb_experiment_amd import nn as rnn
    assert MODELS["pna"] is PNA and "pna" not in REGISTRY
    assert "pna" not in dist_experiment.SUPPORTED
    assert len(InitialParameters.model_names) == 13
    assert "PNAConv" in rnn.__all__


@pytest.mark.parametrize("edge_dim", [None, 3])
@pytest.mark.parametrize("towers", [1, 4])
def test_state_dict_layout_is_pygs(towers, edge_dim):
    conv = PNAConv(8, 12, ["mean", "max", "min", "std"], ["identity", "amplification", "attenuation"], deg=None,
                   edge_dim=edge_dim, towers=towers, post_layers=2)
    Fi, Fo = 8, 12 // towers
    shapes = {"lin.weight": (12, 12), "lin.bias": (12,)}
    for t in range(towers):
        shapes.update({f"pre_nns.{t}.0.weight": (Fi, (3 if edge_dim else 2) * Fi), f"pre_nns.{t}.0.bias": (Fi,),
                       f"post_nns.{t}.0.weight": (Fo, 13 * Fi), f"post_nns.{t}.0.bias": (Fo,),
                       f"post_nns.{t}.2.weight": (Fo, Fo), f"post_nns.{t}.2.bias": (Fo,)})
    if edge_dim:
        shapes.update({"edge_encoder.weight": (Fi, edge_dim), "edge_encoder.bias": (Fi,)})
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == shapes      # the averages are not in it
    assert tuple(conv.avg_deg.shape) == (2,) and "avg_deg" in dict(conv.named_buffers())
    ref = RefPNAConv(8, 12, DEFAULT_AGGR, DEFAULT_SCALERS, (1.0, 1.0), edge_dim, towers, 2)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    divided = PNAConv(8, 12, ["sum"], ["identity"], towers=4, divide_input=True)
    assert tuple(divided.state_dict()["pre_nns.3.0.weight"].shape) == (2, 4)
    assert tuple(divided.state_dict()["post_nns.0.0.weight"].shape) == (3, 4)


def test_deg_histogram_gives_pygs_averages():
    ei = layer_graph()
    hist = torch.bincount(torch.bincount(ei[1], minlength=LAYER_N))
    conv = PNAConv(8, 8, ["mean"], ["identity"], deg=hist)
    assert torch.allclose(conv.avg_deg, averages_of(ei, LAYER_N), rtol=1e-6, atol=0) and conv._avg_known
    assert not PNAConv(8, 8, ["mean"], ["identity"])._avg_known                     # deg=None: the first graph seen


def test_model_layout():
    model = PNA(10, 5, 8, 3, 0.5, towers=4, edge_dim=6, post_layers=2)
    assert inspect.getfullargspec(PNA.__init__).args[1:] == ["input_dim", "output_dim", "hidden_unit", "num_layers",
                                                             "dropout_rate", "aggregators", "scalers", "towers",
                                                             "edge_dim", "post_layers"]
    assert inspect.getfullargspec(PNA.__init__).defaults == (DEFAULT_AGGR, DEFAULT_SCALERS, 1, None, 1)
    assert [c.towers for c in model.convs] == [4, 4, 1] and all(isinstance(c, PNAConv) for c in model.convs)
    assert [(c.in_channels, c.out_channels) for c in model.convs] == [(10, 8), (8, 8), (8, 5)]
    assert inspect.getfullargspec(PNAConv.__init__).args[1:12] == [
        "in_channels", "out_channels", "aggregators", "scalers", "deg", "edge_dim", "towers", "pre_layers", "post_layers",
        "divide_input", "act"]


def test_layer_model_and_operator_refusals():
    from rgb_experiment_amd import ops
    from rgb_experiment_amd.graph import LOOPS_ADD_REMAINING, LOOPS_REMOVE_ADD
    aggr, sc = ["mean", "max"], ["identity", "linear"]
    with pytest.raises(NotImplementedError, match="pre_layers"):
        PNAConv(8, 8, aggr, sc, pre_layers=2)
    with pytest.raises(NotImplementedError, match="train_norm"):
        PNAConv(8, 8, aggr, sc, train_norm=True)
    with pytest.raises(NotImplementedError, match="aggr"):
        PNAConv(8, 8, ["median"], sc)
    with pytest.raises(NotImplementedError, match="scalers"):
        PNAConv(8, 8, aggr, ["exponential"])
    with pytest.raises(ValueError, match="towers"):
        PNAConv(8, 10, aggr, sc, towers=4)
    with pytest.raises(ValueError, match="towers"):
        PNAConv(10, 8, aggr, sc, towers=4, divide_input=True)
    x, ei = torch.randn(5, 8), torch.tensor([[0, 1, 2], [1, 2, 3]])
    conv, edged = PNAConv(8, 8, aggr, sc), PNAConv(8, 8, aggr, sc, edge_dim=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(x, ei)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        edged(x, ei, torch.randn(3, 3))
    with pytest.raises(ValueError, match="edge_attr"):
        edged(x, ei, torch.randn(3, 4))
    with pytest.raises(ValueError, match="edge_attr"):
        edged(x, ei)
    with pytest.raises(ValueError, match="edge_attr"):
        conv(x, ei, torch.randn(3, 3))
    with pytest.raises(ValueError, match="in_channels"):
        conv(torch.randn(5, 6), ei)
    with pytest.raises(ValueError, match="num_layers"):
        PNA(8, 4, 8, 0, 0.0)
    with pytest.raises(ValueError, match="edge_attr"):
        PNA(8, 4, 8, 2, 0.0, edge_dim=3)(x, ei)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PNA(8, 4, 8, 2, 0.0)(x, ei)

    class Partitioned:
        is_distributed = True
    t, avg = torch.zeros(4, 8), torch.ones(2)
    with pytest.raises(RuntimeError, match="no node-partitioned form"):
        ops.pna_aggregate(t, t, None, Partitioned(), aggr, sc, avg, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pna_aggregate(t, t, None, object(), aggr, sc, avg, 8)
    assert ops.PNA_SCALERS == {"identity": 0, "amplification": 1, "attenuation": 2, "linear": 3, "inverse_linear": 4}
    with pytest.raises(ValueError, match="scalers"):
        ops.pna_scaler_names(["identity", "identity"])
    for mode in (LOOPS_ADD_REMAINING, LOOPS_REMOVE_ADD):   # the mode check stands in front of every launch
        src = inspect.getsource(ops.pna_aggregate)
        assert src.index("LOOPS_KEEP") < src.index("_PNAAggregate.apply")


PNA_INIT = {"num_layers": 2, "hidden_unit": 8, "dropout_rate": 0.0}


def test_experiment_flag_checks():
    run, data = G._run, G._data
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # admitted by the flag: the device check is next
        run(data(True), model_name="pna", init={**PNA_INIT, "edge_dim": 4}, use_edge_attr=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # and runs without it
        run(data(False), model_name="pna", init=PNA_INIT)
    with pytest.raises(NotImplementedError, match="partitioned"):
        run(data(True), model_name="pna", init={**PNA_INIT, "edge_dim": 4}, use_edge_attr=True, distributed=True)
    with pytest.raises(ValueError, match="to_undirected"):
        run(data(True), model_name="pna", init={**PNA_INIT, "edge_dim": 4}, use_edge_attr=True, to_undirected_graph=True)
    with pytest.raises(ValueError, match="needs data.edge_attr"):
        run(data(False), model_name="pna", init={**PNA_INIT, "edge_dim": 4}, use_edge_attr=True)
    with pytest.raises(NotImplementedError):                                   # the name checks stay in front
        run(data(True), model_name="fagcn", use_edge_attr=True)
    with pytest.raises(ValueError, match="unknown model_name"):
        run(data(True), model_name="nonesuch", use_edge_attr=True)
    with pytest.raises(ValueError, match="takes no edge attributes.*pna"):
        run(data(True), model_name="gcn", use_edge_attr=True)
    import rgb_experiment_amd
    assert "pna" in inspect.getdoc(rgb_experiment_amd.experiment)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

NEW_ENTRIES = ("rgbx_pna_supported", "rgbx_pna_partial_words", "rgbx_pna_fwd_f32", "rgbx_pna_bwd_src_f32",
               "rgbx_pna_bwd_edge_f32")


def test_abi_declares_and_exports_the_new_entries():
    import ctypes
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
    for d in range(0, 300):
        for F in (0, 2, 4, 6, 8, 12, 16, 64, 256):
            want = d % 4 == 0 and 4 <= d <= 256 and F >= 4 and F % 4 == 0 and d % F == 0
            assert bool(lib.rgbx_pna_supported(d, F)) == want, (d, F)
    words = ctypes.c_int64(-1)
    assert lib.rgbx_pna_partial_words(10, 64, 63, ctypes.byref(words)) == 0 and words.value == 10 * 64 * 8
    assert lib.rgbx_pna_partial_words(10, 64, 2 | 16, ctypes.byref(words)) == 0 and words.value == 10 * 64 * 3
    assert lib.rgbx_pna_partial_words(10, 64, 8, ctypes.byref(words)) == 0 and words.value == 10 * 64 * 3
    assert lib.rgbx_pna_partial_words(10, 64, 0, ctypes.byref(words)) == -1
    assert lib.rgbx_pna_partial_words(10, 64, 63, None) == -1
    p = 0x10000  # 16-byte aligned, non-null, never dereferenced: every call below returns before a launch
    kinds = (ctypes.c_int32 * 3)(0, 1, 2)
    order = (ctypes.c_int32 * 4)(2, 16, 32, 8)

    def fwd(**kw):
        a = dict(rowptr=p, col=p, a=p, lda=64, b=p, ldb=64, c=p, ldc=64, avg=p, which=2 | 8 | 16 | 32, order=order,
                 scalers=kinds, S=3, out=p + 4096, ld_out=64 * 12, mean=None, std=None, argmax=None, argmin=None, N=10, d=64,
                 F=64, split=None, words=0)
        a.update(kw)
        o = _lib.PnaOut()
        o.out, o.ld_out = a["out"], a["ld_out"]
        for k in ("mean", "std", "argmax", "argmin"):
            setattr(o, k, a[k])
            setattr(o, "ld_" + k, 64)
        return lib.rgbx_pna_fwd_f32(a["rowptr"], a["col"], a["a"], a["lda"], a["b"], a["ldb"], a["c"], a["ldc"], a["avg"],
                                    a["which"], a["order"], a["scalers"], a["S"], ctypes.byref(o), a["N"], a["d"], a["F"],
                                    a["split"], a["words"], None)
    assert fwd(rowptr=None) == -1 and b"null" in lib.rgbx_last_error_string()
    assert fwd(col=None) == -1 and fwd(b=None) == -1 and fwd(avg=None) == -1 and fwd(out=None) == -1
    assert fwd(scalers=None) == -1
    assert fwd(which=0) == -1 and b"aggregator" in lib.rgbx_last_error_string()          # no aggregator
    assert fwd(S=0) == -1 and b"scaler" in lib.rgbx_last_error_string()                  # no scaler
    assert fwd(scalers=(ctypes.c_int32 * 3)(0, 1, 7)) == -1
    assert fwd(which=2 | 8, order=None, argmax=p) == -1 and b"extremum" in lib.rgbx_last_error_string()
    assert fwd(which=2 | 8, order=None, argmin=p) == -1
    assert fwd(which=16, order=None, std=p) == -1 and fwd(which=16, order=None, mean=p) == -1
    assert fwd(order=(ctypes.c_int32 * 4)(2, 16, 16, 8)) == -1 and b"aggr_order" in lib.rgbx_last_error_string()
    assert fwd(order=(ctypes.c_int32 * 4)(2, 16, 1, 8)) == -1
    assert fwd(ldb=32) == -1 and fwd(ldc=60) == -1 and fwd(lda=8) == -1 and fwd(ld_out=64 * 12 - 4) == -1
    assert fwd(N=-1) == -1 and fwd(N=2 ** 31) == -2                                      # RGBX_E_RANGE
    assert fwd(d=64, F=24) == -5 and b"F" in lib.rgbx_last_error_string()                # RGBX_E_SHAPE: F does not divide d
    assert fwd(d=66, F=66) == -5 and fwd(d=260, F=4) == -5 and fwd(d=64, F=6) == -5 and fwd(d=0, F=4) == -5
    assert fwd(b=p + 4) == -3 and b"aligned" in lib.rgbx_last_error_string()             # RGBX_E_ALIGN
    assert fwd(c=p + 8) == -3 and fwd(a=p + 4) == -3 and fwd(out=p + 4100) == -3 and fwd(ldb=66) == -3
    assert fwd(mean=p + 4) == -3 and fwd(argmax=p + 8) == -3 and fwd(avg=p + 2) == -3
    split = _lib.RowSplit(1024, 3, 1, p, p, p, p, p, p)
    assert fwd(split=ctypes.byref(split), words=3 * 64 * 8 - 1) == -4                    # RGBX_E_WS: mean, std (three sections), max, min (two each)
    assert b"partial" in lib.rgbx_last_error_string()
    assert fwd(split=ctypes.byref(split), words=3 * 64 * 8 - 1, mean=p) == -4
    bad = _lib.RowSplit(1024, 3, 1, p, p, p, p, p, p + 4)
    assert fwd(split=ctypes.byref(bad), words=10 ** 6) == -1
    assert fwd(out=p) == -1 and b"alias" in lib.rgbx_last_error_string()
    assert fwd(N=0) == 0

    def terms(**kw):
        a = dict(A=p, B=p, gmax=p, argmax=p, gmin=p, argmin=p, ld=64)
        a.update(kw)
        t = _lib.PnaGrad()
        for k in ("A", "B", "gmax", "argmax", "gmin", "argmin"):
            setattr(t, k, a[k])
            setattr(t, "ld_" + k, a["ld"])
        return t

    def src(t=None, **kw):
        a = dict(rowptr=p, col=p, t2f=p, b=p, ldb=64, c=p, ldc=64, g=p + 64, ldg=64, N=10, d=64)
        a.update(kw)
        return lib.rgbx_pna_bwd_src_f32(a["rowptr"], a["col"], a["t2f"], a["b"], a["ldb"], a["c"], a["ldc"],
                                        ctypes.byref(t or terms()), a["g"], a["ldg"], a["N"], a["d"], None, None)

    def edge(t=None, **kw):
        a = dict(rowptr=p, col=p, b=p, ldb=64, c=p, ldc=64, g=p + 64, ldg=64, N=10, d=64)
        a.update(kw)
        return lib.rgbx_pna_bwd_edge_f32(a["rowptr"], a["col"], a["b"], a["ldb"], a["c"], a["ldc"],
                                         ctypes.byref(t or terms()), a["g"], a["ldg"], a["N"], a["d"], None, None)
    for fn in (src, edge):
        assert fn(rowptr=None) == -1 and fn(col=None) == -1 and fn(g=None) == -1
        assert fn(terms(A=None, B=None, gmax=None, argmax=None, gmin=None, argmin=None)) == -1
        assert b"no term" in lib.rgbx_last_error_string()
        assert fn(terms(argmax=None)) == -1 and fn(terms(gmin=None)) == -1               # cotangent and arg go together
        assert fn(b=None) == -1                                                           # B needs b
        assert fn(terms(ld=32)) == -1 and fn(ldg=60) == -1 and fn(ldb=8) == -1
        assert fn(g=p) == -1 and b"alias" in lib.rgbx_last_error_string()
        assert fn(N=-1) == -1 and fn(N=2 ** 31) == -2
        wide = dict(ldb=512, ldc=512, ldg=512)
        assert fn(terms(ld=512), d=66, **wide) == -5 and fn(terms(ld=512), d=260, **wide) == -5
        assert fn(terms(A=p + 4)) == -3 and fn(terms(argmin=p + 8)) == -3 and fn(g=p + 68) == -3 and fn(b=p + 4) == -3
        assert fn(N=0) == 0
    assert src(t2f=None) == -1 and b"t2f" in lib.rgbx_last_error_string()
    assert edge(c=None) == -1                                                             # the edge pass needs c with B
    assert src(terms(B=None), b=None, c=None, N=0) == 0 and src(c=None, N=0) == 0         # c may be NULL on the source side
