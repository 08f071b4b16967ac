"""Softmax and log-sum-exp at trained score ranges, host side: the case builders tests/test_gpu_softmax_range.py feeds
to the HIP kernels, and the checks that keep those cases in the regime they exist for. No GPU needed.

Every attention case is an order-1 case of the existing operator tests (same graphs, same shapes, float64 inputs that
float32 holds exactly) whose attention vectors — for GAT's operator form the scores a_src / a_dst themselves — are
multiplied by a scale, so that the scores reach a few hundred while the features, and with them max(1, |ref|max) of
`close`, stay where they were. The scales and seeds below were chosen on the CPU from the float64 restatements alone.

What a family of cases has to show (score_profile measures it, the tests below assert it and print it):
  overflow    a row maximum >= 100 (> log FLT_MAX = 88.7: an unshifted expf(e) is inf)
  low row     a row whose scores are all <= -100 (the running maximum's start value must act as minus infinity)
  underflow   an edge with e - rowmax <= -110 (its float32 weight is exactly 0)
  subnormal   an edge with e - rowmax in [-103, -88] (its float32 weight is subnormal)
  late spike  >= 20 rows of >= 65 slots whose maximum sits in the last quarter of the row's CSR slot order and >= 40
              above everything before it (the accumulator is rescaled after it has filled)
  chunks      on rows cut into chunks of LONG_ROW_SLOTS, over the heads: the row maximum in the first chunk for one
              head and in the last chunk for another, with chunk maxima >= 40 apart (the combine of unequal states)
  saturated   >= 5 % of the (row, head) pairs with >= 2 slots have one weight > 0.999
  well-posed  the same formulas in float32 on the CPU agree with float64 within a QUARTER of the tolerance the GPU test
              uses (forward 2.5e-5, gradients 5e-5, times max(1, |ref|max)): a condition on the inputs, not on a kernel

A property is asserted per FAMILY (GATv2, GAT, SuperGAT): over its cases, since no single case can show all of them — the
graphs `random` and `hub` have one row of 65 slots between them, a single-head case has one maximum per hub row, and a
SuperGAT case of one (even) head has negative scores only. Overflow / underflow / subnormal / saturation and
well-posedness are asserted for every case. Where the existing construction cannot reach a property, the case says so
where it departs from "the order-1 case times a scale": `powerlaw` joins GAT's and SuperGAT's graphs (late spikes),
GAT's target-side scores and SuperGAT's even heads carry a larger scale (LeakyReLU's 0.2), SuperGAT gets a few spike
sources, and the per-edge softmax — whose bar is absolute — gets scores on a grid.

The slot order of a row is the oracle's CSR (stable grouping of the rewritten edge list by target), which the device's
CSR equals bit for bit (tests/test_gpu_parity.py::test_csr_build_bit_exact).

LeakyReLU's kink stays out of every gradient comparison: GATv2's s = xl + xr and GAT's s = a_src + a_dst are one exact
addition of inputs; gat_attend's vectors carry one channel of power-of-two size per head, so a score is one exact
product; SuperGAT keeps make_case's channel-0 construction and assert_no_kink."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from test_gatv2_host import RefGATv2Conv, rewritten_edges

SLOPE = 0.2
FWD_TOL, GRAD_TOL = 1e-4, 2e-4          # the project's tolerances (tests/test_gpu_gatv2.py), used unchanged on the GPU
WELL_POSED_SHARE = 0.25                 # float32-vs-float64 on the CPU may use this share of them
LONG_ROW_SLOTS = 1024                   # rgb_experiment_amd.graph.LONG_ROW_SLOTS (asserted below)


# ---- graphs -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def graph_of(name):
    """(edge_index, n) of the existing operator tests' graphs, built once."""
    from test_gpu_fagcn import powerlaw_graph
    from test_gpu_ggnn import hub_graph, rand_graph
    if name == "random":
        return rand_graph(700, 6000, 3, loops=11, dups=40), 700
    if name == "hub":
        return hub_graph(1500, 21), 1500
    if name == "powerlaw":
        return powerlaw_graph(), 2000
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def slots_of(name):
    """(src, dst) after the self-loop rewrite, the CSR's (rowptr, order): slot p of the CSR is edge order[p]."""
    ei, n = graph_of(name)
    src, dst = rewritten_edges(ei, n)
    rowptr, _, order = O.csr_from_edges(dst, src, torch.arange(dst.numel()), n)
    return src, dst, rowptr.long(), order.long()


def f32_exact(t):
    """float64 copy of a tensor rounded to float32: both sides of a comparison hold the same numbers."""
    return t.float().double()


# ---- what a set of scores exercises -------------------------------------------------------------------------------------

def score_profile(e, graph_name):
    """`e` [E', H] float64 in edge order (rewritten_edges) -> the measurements of the module docstring."""
    _, n = graph_of(graph_name)
    src, dst, rowptr, order = slots_of(graph_name)
    e = e.detach()
    H = e.size(1)
    idx = dst.view(-1, 1).expand(-1, H)
    rowmax = torch.full((n, H), -1e30, dtype=torch.float64).scatter_reduce(0, idx, e, "amax")
    rel = e - rowmax[dst]
    ex = torch.exp(rel)
    alpha = ex / (torch.zeros(n, H, dtype=torch.float64).index_add(0, dst, ex)[dst] + 1e-16)
    top = torch.zeros(n, H, dtype=torch.float64).scatter_reduce(0, idx, alpha, "amax")
    deg = rowptr[1:] - rowptr[:-1]
    multi = deg >= 2
    es = e[order]
    late_rows, chunk_hits = 0, set()
    for r in torch.nonzero(deg >= 65).view(-1).tolist():
        row = es[rowptr[r]:rowptr[r + 1]]                                # [deg, H] in slot order
        k = row.size(0)
        at = row.argmax(0)
        before = torch.cat([torch.full((1, H), -1e30, dtype=torch.float64), torch.cummax(row, 0)[0]])[at, torch.arange(H)]
        hit = (at >= 0.75 * k) & (row.max(0)[0] - before >= 40)
        late_rows += int(hit.any())
        if k > LONG_ROW_SLOTS:
            cmax = torch.stack([c.max(0)[0] for c in row.split(LONG_ROW_SLOTS)])      # [chunks, H]
            apart = cmax.max(0)[0] - cmax.min(0)[0] >= 40
            last = (k - 1) // LONG_ROW_SLOTS
            for h in range(H):
                if apart[h]:
                    c = int(at[h]) // LONG_ROW_SLOTS
                    chunk_hits.add("first" if c == 0 else "last" if c == last else "middle")
    return {
        "max_e": e.max().item(), "min_e": e.min().item(), "max_rowmax": rowmax.max().item(),
        "min_rowmax": rowmax.min().item(), "min_rel": rel.min().item(),
        "underflow": int((rel <= -110).sum()), "subnormal": int(((rel >= -103) & (rel <= -88)).sum()),
        "late_rows": late_rows, "chunks": chunk_hits,
        "saturated": (top[multi] > 0.999).double().mean().item(),
    }


PROPERTIES = {
    "overflow": lambda p: p["max_rowmax"] >= 100,
    "low row": lambda p: p["min_rowmax"] <= -100,
    "underflow": lambda p: p["underflow"] >= 1,
    "subnormal": lambda p: p["subnormal"] >= 1,
    "late spike": lambda p: p["late_rows"] >= 20,
    "chunks": lambda p: {"first", "last"} <= p["chunks"],
    "saturated": lambda p: p["saturated"] >= 0.05,
}


def union_profile(profiles):
    """The profile of a family: a property counts where one case shows it; the chunk positions add up over the cases
    (a single-head case has one maximum per hub row)."""
    out = {k: max(p[k] for p in profiles) for k in ("max_e", "max_rowmax", "underflow", "subnormal", "late_rows", "saturated")}
    out.update({k: min(p[k] for p in profiles) for k in ("min_e", "min_rowmax", "min_rel")})
    out["chunks"] = set().union(*(p["chunks"] for p in profiles))
    return out


def show(name, p, shares=None):
    line = (f"{name}: max e {p['max_e']:.1f}, min e {p['min_e']:.1f}, highest row max {p['max_rowmax']:.1f}, lowest row max "
            f"{p['min_rowmax']:.1f}, min e - rowmax {p['min_rel']:.1f} ({p['underflow']} underflow, {p['subnormal']} subnormal), "
            f"late-spike rows {p['late_rows']}, hub maxima in chunks {sorted(p['chunks'])}, saturated {p['saturated']:.2f}")
    if shares is not None:
        line += "; float32 vs float64 share of tolerance " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items())
    print(line)


def share_of_tolerance(got, want, tol):
    """max |got - want| as a share of tol * max(1, |want|max): `close` passes below 1."""
    return (got.detach().double() - want.detach()).abs().max().item() / (tol * max(1.0, want.detach().abs().max().item()))


def segment_softmax(e, dst, n):
    """PyG's softmax per target, in e's own precision (RefGATv2Conv.attend's lines, any dtype)."""
    H = e.size(1)
    idx = dst.view(-1, 1).expand(-1, H)
    mx = torch.full((n, H), -1e30, dtype=e.dtype).scatter_reduce(0, idx, e.detach(), "amax")
    ex = torch.exp(e - mx[dst])
    den = torch.zeros(n, H, dtype=e.dtype).index_add(0, dst, ex)
    return ex / (den[dst] + 1e-16)


def _leaves(dtype, *tensors):
    return [t.to(dtype).clone().requires_grad_(True) for t in tensors]


# ---- GATv2 ------------------------------------------------------------------------------------------------------------

GATV2_PAIRS = [(1, 4), (8, 8), (8, 40), (1, 64), (1, 256)]
GATV2_GRAPHS = ("random", "powerlaw")
# (H, C, graph) -> (seed of operator_case, scale of att)
GATV2_PLAN = {(H, C, g): (1000 + 10 * H + C, 70.0) for H, C in GATV2_PAIRS for g in GATV2_GRAPHS}
# seeds 1000 ... scanned for the chunk property on the one row of `powerlaw` above LONG_ROW_SLOTS (1756 slots, 2 chunks)
GATV2_PLAN[(8, 8, "powerlaw")] = (1000, 70.0)
GATV2_PLAN[(8, 40, "powerlaw")] = (1030, 70.0)


@functools.lru_cache(maxsize=None)
def gatv2_case(H, C, graph_name):
    """xl, xr [n, H*C], att [1, H, C] (operator_case's, times the scale), bias [H*C], cotangent: float64, fp32-exact."""
    from test_gpu_gatv2 import operator_case
    _, n = graph_of(graph_name)
    seed, scale = GATV2_PLAN[(H, C, graph_name)]
    xl, xr, att, bias, cot = operator_case(H, C, n, seed)
    return xl, xr, f32_exact(att.float() * scale), bias, cot


def gatv2_formula(xl, xr, att, bias, cot, src, dst, n, H, C, keep=None, p=0.0):
    """GATv2's attention in the precision of its inputs: (out, [g_xl, g_xr, g_att, g_bias], e)."""
    xl, xr, att, bias = _leaves(xl.dtype, xl, xr, att, bias)
    s = xl.view(n, H, C)[src] + xr.view(n, H, C)[dst]
    e = (att * F.leaky_relu(s, SLOPE)).sum(-1)
    alpha = segment_softmax(e, dst, n)
    if keep is not None:
        alpha = alpha * keep.to(e.dtype) / (1.0 - p)
    out = torch.zeros(n, H, C, dtype=e.dtype).index_add(0, dst, alpha.unsqueeze(-1) * xl.view(n, H, C)[src])
    out = out.reshape(n, H * C) + bias
    (out * cot.to(e.dtype)).sum().backward()
    return out.detach(), [xl.grad, xr.grad, att.grad, bias.grad], e.detach()


def gatv2_reference(H, C, graph_name, src, dst, keep=None, p=0.0):
    """The project's float64 restatement (RefGATv2Conv.attend) on a case: (out, [g_xl, g_xr, g_att, g_bias], e)."""
    _, n = graph_of(graph_name)
    xl, xr, att, bias, cot = gatv2_case(H, C, graph_name)
    ref = RefGATv2Conv(1, C, heads=H, negative_slope=SLOPE, dropout=p)
    xl_r, xr_r, bias_r = (t.clone().requires_grad_(True) for t in (xl, xr, bias))
    with torch.no_grad():
        ref.att.copy_(att)
    want = ref.attend(xl_r.view(n, H, C), xr_r.view(n, H, C), n, src, dst, keep).reshape(n, H * C) + bias_r
    (want * cot).sum().backward()
    return want.detach(), [xl_r.grad, xr_r.grad, ref.att.grad, bias_r.grad], ref.e


@functools.lru_cache(maxsize=None)
def gatv2_eval_reference(H, C, graph_name):
    src, dst, _, _ = slots_of(graph_name)
    return gatv2_reference(H, C, graph_name, src, dst)


def shares_of(got, want, names):
    """{name: share of the GPU test's tolerance}: the first entry is the forward, the others gradients."""
    out = {names[0]: share_of_tolerance(got[0], want[0], FWD_TOL)}
    for k, a, b in zip(names[1:], got[1], want[1]):
        out[k] = share_of_tolerance(a, b, GRAD_TOL)
    return out


GATV2_NAMES = ("forward", "g_xl", "g_xr", "g_att", "g_bias")


@pytest.mark.parametrize("graph", GATV2_GRAPHS)
@pytest.mark.parametrize("H,C", GATV2_PAIRS)
def test_gatv2_case_is_in_range_and_well_posed(H, C, graph):
    """Per case: the scores are far outside order 1 (overflow, underflow, saturation hold in EVERY case), the formula
    of this module is the project's restatement, and float32 stays inside a quarter of the tolerance."""
    _, n = graph_of(graph)
    src, dst, _, _ = slots_of(graph)
    want = gatv2_eval_reference(H, C, graph)
    prof = score_profile(want[2], graph)
    case = gatv2_case(H, C, graph)
    same = gatv2_formula(*case, src, dst, n, H, C)
    assert max(shares_of(same, want, GATV2_NAMES).values()) < 1e-6, "this module's formula is not the restatement's"
    low = gatv2_formula(*(t.float() for t in case), src, dst, n, H, C)
    assert all(torch.isfinite(t).all() for t in [low[0]] + low[1])
    shares = shares_of(low, want, GATV2_NAMES)
    show(f"gatv2 ({H}, {C}) {graph}", prof, shares)
    for name in ("overflow", "underflow", "subnormal", "saturated"):
        assert PROPERTIES[name](prof), name
    assert max(shares.values()) <= WELL_POSED_SHARE, shares


def test_gatv2_family_shows_every_property():
    profs = [score_profile(gatv2_eval_reference(H, C, g)[2], g) for H, C in GATV2_PAIRS for g in GATV2_GRAPHS]
    fam = union_profile(profs)
    show("gatv2 family", fam)
    for name, holds in PROPERTIES.items():
        assert holds(fam), name
    # the chunk property inside ONE multi-head case, as the combine kernel meets it in one launch
    assert any({"first", "last"} <= p["chunks"] for p in profs)


def test_long_row_threshold_is_the_products():
    from rgb_experiment_amd import graph as G
    assert G.LONG_ROW_SLOTS == LONG_ROW_SLOTS
    for name in ("hub", "powerlaw"):
        rowptr = slots_of(name)[2]
        chunks = -(-int((rowptr[1:] - rowptr[:-1]).max()) // LONG_ROW_SLOTS)
        assert chunks == {"hub": 3, "powerlaw": 2}[name]


# ---- GAT --------------------------------------------------------------------------------------------------------------

GAT_PAIRS = [(8, 8), (1, 7), (8, 16), (1, 128)]
# `powerlaw` is here for the late-spike property: `random` and `hub` have no 20 rows of 65 slots
GAT_GRAPHS = ("random", "hub", "powerlaw")
# LeakyReLU compresses the negative side by 0.2: a row whose scores are ALL <= -100 needs a_dst <= -500 - max a_src, so
# the target-side scores carry the larger scale (they shift a whole row), the source-side scores spread it
GAT_SRC_SCALE, GAT_DST_SCALE = 70.0, 200.0
# (H, C, graph) -> seed
GAT_PLAN = {(H, C, g): 2000 + 10 * H + C for H, C in GAT_PAIRS for g in GAT_GRAPHS}
# seeds 2000 ... scanned for the chunk property on the hub row (2501 slots, 3 chunks)
GAT_PLAN[(8, 8, "hub")] = 2018
GAT_PLAN[(8, 16, "hub")] = 2001


@functools.lru_cache(maxsize=None)
def gat_case(H, C, graph_name):
    """ops.gat_aggregate's operands: h [n, H*C] of order 1, a_src, a_dst [n, H] scaled, cotangent; float64, fp32-exact."""
    _, n = graph_of(graph_name)
    g = torch.Generator().manual_seed(GAT_PLAN[(H, C, graph_name)])
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    return (rnd(n, H * C).double(), f32_exact(rnd(n, H) * GAT_SRC_SCALE), f32_exact(rnd(n, H) * GAT_DST_SCALE),
            rnd(n, H * C).double())


def gat_formula(h, a_src, a_dst, cot, src, dst, n, H, C):
    """GAT's aggregation from given scores with the oracle's segment softmax, in the precision of the inputs:
    (out, [g_h, g_a_src, g_a_dst], e)."""
    h, a_src, a_dst = _leaves(h.dtype, h, a_src, a_dst)
    e = F.leaky_relu(a_src[src] + a_dst[dst], SLOPE)
    alpha = O.segment_softmax(e, dst, n)
    out = torch.zeros(n, H, C, dtype=e.dtype).index_add(0, dst, alpha.unsqueeze(-1) * h.view(n, H, C)[src])
    out = out.reshape(n, H * C)
    (out * cot.to(e.dtype)).sum().backward()
    return out.detach(), [h.grad, a_src.grad, a_dst.grad], e.detach()


@functools.lru_cache(maxsize=None)
def gat_reference(H, C, graph_name):
    _, n = graph_of(graph_name)
    src, dst, _, _ = slots_of(graph_name)
    return gat_formula(*gat_case(H, C, graph_name), src, dst, n, H, C)


GAT_NAMES = ("forward", "g_h", "g_a_src", "g_a_dst")


@pytest.mark.parametrize("graph", GAT_GRAPHS)
@pytest.mark.parametrize("H,C", GAT_PAIRS)
def test_gat_case_is_in_range_and_well_posed(H, C, graph):
    _, n = graph_of(graph)
    src, dst, _, _ = slots_of(graph)
    want = gat_reference(H, C, graph)
    prof = score_profile(want[2], graph)
    low = gat_formula(*(t.float() for t in gat_case(H, C, graph)), src, dst, n, H, C)
    assert all(torch.isfinite(t).all() for t in [low[0]] + low[1])
    shares = shares_of(low, want, GAT_NAMES)
    show(f"gat ({H}, {C}) {graph}", prof, shares)
    for name in ("overflow", "underflow", "subnormal", "saturated"):
        assert PROPERTIES[name](prof), name
    assert max(shares.values()) <= WELL_POSED_SHARE, shares


def test_gat_family_shows_every_property():
    profs = {(H, C, g): score_profile(gat_reference(H, C, g)[2], g) for H, C in GAT_PAIRS for g in GAT_GRAPHS}
    fam = union_profile(list(profs.values()))
    show("gat family", fam)
    for name, holds in PROPERTIES.items():
        assert holds(fam), name
    assert any({"first", "last"} <= p["chunks"] for (H, C, g), p in profs.items() if g == "hub")


# ops.gat_attend forms the scores from h and the attention vectors inside the kernel (C = 16) or in a scores launch
# (C = 128): one channel per head carries +-2^6 (source) / +-2^7 (target), the others are zero, so a score is ONE exact
# product in any summation order and LeakyReLU's branch is the float64 branch
GAT_ATTEND_PAIRS = [(8, 16), (1, 128)]
GAT_ATTEND_GRAPHS = ("random", "hub")


@functools.lru_cache(maxsize=None)
def gat_attend_case(H, C, graph_name):
    """h [n, H*C], att_src, att_dst [1, H, C] (one power-of-two channel per head), bias [H*C], cotangent."""
    _, n = graph_of(graph_name)
    g = torch.Generator().manual_seed(3000 + 10 * H + C)
    h = torch.randn(n, H * C, generator=g).double()
    att = torch.zeros(2, 1, H, C, dtype=torch.float64)
    for k, size in enumerate((64.0, 128.0)):
        ch = torch.randint(0, C, (H,), generator=g)
        sign = torch.randint(0, 2, (H,), generator=g).double() * 2 - 1
        att[k, 0, torch.arange(H), ch] = sign * size
    return h, att[0], att[1], torch.randn(H * C, generator=g).double(), torch.randn(n, H * C, generator=g).double()


def gat_attend_formula(h, att_src, att_dst, bias, cot, src, dst, n, H, C):
    """(out, [g_h, g_att_src, g_att_dst, g_bias], e) in the precision of the inputs."""
    h, att_src, att_dst, bias = _leaves(h.dtype, h, att_src, att_dst, bias)
    h3 = h.view(n, H, C)
    a_src, a_dst = (h3 * att_src).sum(-1), (h3 * att_dst).sum(-1)
    e = F.leaky_relu(a_src[src] + a_dst[dst], SLOPE)
    alpha = O.segment_softmax(e, dst, n)
    out = torch.zeros(n, H, C, dtype=e.dtype).index_add(0, dst, alpha.unsqueeze(-1) * h3[src]).reshape(n, H * C) + bias
    (out * cot.to(e.dtype)).sum().backward()
    return out.detach(), [h.grad, att_src.grad, att_dst.grad, bias.grad], e.detach()


@functools.lru_cache(maxsize=None)
def gat_attend_reference(H, C, graph_name):
    _, n = graph_of(graph_name)
    src, dst, _, _ = slots_of(graph_name)
    return gat_attend_formula(*gat_attend_case(H, C, graph_name), src, dst, n, H, C)


GAT_ATTEND_NAMES = ("forward", "g_h", "g_att_src", "g_att_dst", "g_bias")


@pytest.mark.parametrize("graph", GAT_ATTEND_GRAPHS)
@pytest.mark.parametrize("H,C", GAT_ATTEND_PAIRS)
def test_gat_attend_case_is_in_range_and_well_posed(H, C, graph):
    ei, n = graph_of(graph)
    src, dst, _, _ = slots_of(graph)
    case = gat_attend_case(H, C, graph)
    want = gat_attend_reference(H, C, graph)
    # the formula is the oracle's GATConv behind an identity projection
    oracle = O.gat_conv(case[0], ei, torch.eye(H * C, dtype=torch.float64), case[1], case[2], case[3], H, True)
    assert (oracle - want[0]).abs().max().item() < 1e-12
    # one exact product per score: float32 holds the float64 scores
    h3 = case[0].view(n, H, C)
    for att in case[1:3]:
        assert int((att != 0).sum()) == H
        assert torch.equal((h3.float() * att.float()).sum(-1).double(), (h3 * att).sum(-1))
    prof = score_profile(want[2], graph)
    low = gat_attend_formula(*(t.float() for t in case), src, dst, n, H, C)
    shares = shares_of(low, want, GAT_ATTEND_NAMES)
    show(f"gat_attend ({H}, {C}) {graph}", prof, shares)
    for name in ("overflow", "underflow", "subnormal", "saturated"):
        assert PROPERTIES[name](prof), name
    assert max(shares.values()) <= WELL_POSED_SHARE, shares


# ops.gat_attend_linear: one head, the transform behind the aggregation; its scores are float32 products over K = 64
# inputs, so only the forward is compared (continuous across the kink)
GAT_LINEAR_F, GAT_LINEAR_C, GAT_LINEAR_SCALE = 64, 64, 40.0


@functools.lru_cache(maxsize=None)
def gat_linear_case(graph_name="hub"):
    """x [n, 64], W [64, 64] (rows of norm ~1), att_src, att_dst [1, 1, 64] (scores of standard deviation ~SCALE), bias."""
    _, n = graph_of(graph_name)
    g = torch.Generator().manual_seed(3500)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    f, C = GAT_LINEAR_F, GAT_LINEAR_C
    return (rnd(n, f).double(), f32_exact(rnd(C, f) / f ** 0.5), f32_exact(rnd(1, 1, C) * GAT_LINEAR_SCALE / C ** 0.5),
            f32_exact(rnd(1, 1, C) * GAT_LINEAR_SCALE / C ** 0.5), rnd(C).double())


def gat_linear_formula(x, W, att_src, att_dst, bias, ei):
    """(out, e) of the oracle's single-head GATConv in the precision of the inputs."""
    n = x.size(0)
    h = x @ W.t()
    src, dst = rewritten_edges(ei, n)
    e = F.leaky_relu((h * att_src.view(1, -1)).sum(-1)[src] + (h * att_dst.view(1, -1)).sum(-1)[dst], SLOPE).view(-1, 1)
    return O.gat_conv(x, ei, W, att_src, att_dst, bias, 1, False), e


def test_gat_linear_case_is_in_range_and_well_posed():
    ei, n = graph_of("hub")
    case = gat_linear_case("hub")
    want, e = gat_linear_formula(*case, ei)
    prof = score_profile(e, "hub")
    low, _ = gat_linear_formula(*(t.float() for t in case), ei)
    share = share_of_tolerance(low, want, FWD_TOL)
    show("gat_attend_linear (1, 64) hub", prof, {"forward": share})
    for name in ("overflow", "underflow", "subnormal", "saturated"):
        assert PROPERTIES[name](prof), name
    assert share <= WELL_POSED_SHARE, share


# ---- masked cross-entropy -------------------------------------------------------------------------------------------------

LOSS_CLASSES = [1, 7, 40, 47, 130]   # 40: the loss kernels' float4 form (C % 4 == 0)
LOSS_N, LOSS_SCALE, LOSS_SHIFT = 3001, 40.0, 300.0
LOSS_LOW_ROWS, LOSS_HIGH_ROWS = slice(10, 20), slice(20, 30)
LOSS_SURE_ROWS, LOSS_LOST_ROWS, LOSS_TARGET_SHIFT = range(30, 40), range(40, 50), 600.0


@functools.lru_cache(maxsize=None)
def loss_case(C):
    """tests/test_gpu_rows.py::test_row_kernel_cross_entropy's setup with h and bias times LOSS_SCALE: (edge_index,
    h [n, 2d] float32 — columns :d are gathered, columns d: are the additive operand —, bias [d], y, mask). Ten selected
    rows lie LOSS_SHIFT below and ten above the rest (a softmax does not see the shift; its float32 evaluation does);
    ten have their target's logit raised by LOSS_TARGET_SHIFT (probability 1, gradient exactly 0 in float32), ten have it
    lowered as far (probability 0: loss of several hundred, gradient -1 on the target)."""
    from test_gpu_rows import graph_with_isolated_nodes
    n, d = LOSS_N, (C + 3) // 4 * 4
    ei = graph_with_isolated_nodes(n, 25000, C, hub=1200)
    gen = torch.Generator().manual_seed(C)
    h = torch.randn(n, 2 * d, generator=gen) * LOSS_SCALE
    h[:, C:d] = 0  # pad columns, as pad_rows4 produces them
    h[LOSS_LOW_ROWS, d:] -= LOSS_SHIFT
    h[LOSS_HIGH_ROWS, d:] += LOSS_SHIFT
    bias = F.pad(torch.randn(C, generator=gen) * LOSS_SCALE, (0, d - C))
    y = torch.randint(0, C, (n,), generator=gen)
    y[5], y[6] = -1, C  # unlabelled / out of range: deselected
    mask = torch.rand(n, generator=gen) < 0.5
    mask[3] = True  # the hub row
    mask[n - 1] = True  # a node without any edge
    mask[10:50] = True
    for rows, sign in ((LOSS_SURE_ROWS, 1.0), (LOSS_LOST_ROWS, -1.0)):
        for i in rows:
            h[i, d + int(y[i])] += sign * LOSS_TARGET_SHIFT
    return ei, h, bias, y, mask


def host_mean_logits(C):
    """The 'mean' form's logits [n, C] in float64 (what the device forms in float32 inside the gather)."""
    ei, h, bias, _, _ = loss_case(C)
    n, d = LOSS_N, (C + 3) // 4 * 4
    h = h.double()
    deg = torch.bincount(ei[1], minlength=n).double().clamp(min=1).view(-1, 1)
    agg = torch.zeros(n, d, dtype=torch.float64).index_add(0, ei[1], h[ei[0], :d]) / deg
    return (agg + h[:, d:] + bias.double())[:, :C]


def loss_reference(logits, y, mask, C):
    """float64 log_softmax + NLL of float32 logits (taken as exact): (nll sum, selected rows, arg-max hits, the gradient
    softmax - onehot of the SUM of the selected rows' losses [n, C], zero on the other rows)."""
    z = logits.double()
    sel = (y >= 0) & (y < C)
    if mask is not None:
        sel = sel & mask.bool()
    t = y.clamp(0, C - 1)
    logp = F.log_softmax(z, dim=1)
    nll = -logp[torch.arange(z.size(0)), t][sel].sum().item()
    hits = int(((z.argmax(1) == t) & sel).sum())
    grad = (logp.exp() - F.one_hot(t, C).double()) * sel.view(-1, 1).double()
    return nll, int(sel.sum()), hits, grad


def loss_profile(logits, y, mask, C):
    z = logits.double()
    sel = (y >= 0) & (y < C) & mask.bool()
    t = y.clamp(0, C - 1)
    top2 = z.topk(min(2, C), dim=1)[0]
    rel = z - top2[:, :1]
    rel_t = rel[torch.arange(z.size(0)), t]
    return {
        "max": z.max().item(), "min": z.min().item(), "highest_row_max": top2[:, 0].max().item(),
        "lowest_row_max": top2[sel, 0].min().item(), "underflow": int((rel[sel] <= -110).sum()),
        "subnormal": int(((rel[sel] >= -103) & (rel[sel] <= -88)).sum()),
        "target_has_p0": int((rel_t[sel] <= -110).sum()),
        "target_has_p1": int(((rel_t == 0) & (top2[:, -1] - top2[:, 0] <= -110))[sel].sum()) if C > 1 else int(sel.sum()),
        "near_ties": int((top2[sel, 0] - top2[sel, -1] < 1).sum()) if C > 1 else 0,
    }


def assert_loss_profile(p, C):
    """The logits leave order 1 on both sides; with more than one class every band and both extreme rows occur."""
    assert p["highest_row_max"] >= 100 and p["lowest_row_max"] <= -100, p
    if C > 1:
        assert p["max"] >= 150 and p["min"] <= -150, p
        for key in ("underflow", "subnormal", "target_has_p0", "target_has_p1", "near_ties"):
            assert p[key] >= 1, (key, p)


def folded_lse_gradient(z32, y, C):
    """softmax - onehot in float32 with the log-sum-exp FOLDED into one number, lse = max + log(sum): the form whose
    rounding at ulp(|max|) / 2 becomes a relative error of every probability."""
    best = z32.max(1, keepdim=True)[0]
    lse = best + torch.log(torch.exp(z32 - best).sum(1, keepdim=True))
    return torch.exp(z32 - lse) - F.one_hot(y.clamp(0, C - 1), C).float()


@pytest.mark.parametrize("C", LOSS_CLASSES)
def test_loss_case_is_in_range_and_well_posed(C):
    """The issue's bars (NLL sum 1e-5 * max(1, |ref|), gradient 1e-6 absolute) leave float32 four times the room it
    needs when the maximum and log(sum) stay apart; with the two folded into one float32 number the gradient misses
    the bar on these logits — the case tells the two apart."""
    _, _, _, y, mask = loss_case(C)
    z32 = host_mean_logits(C).float()
    prof = loss_profile(z32, y, mask, C)
    nll, count, hits, grad = loss_reference(z32, y, mask, C)
    sel = grad.abs().sum(1) > 0
    lp32 = F.log_softmax(z32, dim=1)
    t = y.clamp(0, C - 1)
    rows = (y >= 0) & (y < C) & mask
    nll32 = -lp32[torch.arange(LOSS_N), t][rows].double().sum().item()
    g32 = (lp32.exp() - F.one_hot(t, C).float()) * rows.view(-1, 1)
    nll_share = abs(nll32 - nll) / (1e-5 * max(1.0, abs(nll)))
    grad_share = (g32.double() - grad).abs().max().item() / 1e-6
    folded = ((folded_lse_gradient(z32, y, C) * rows.view(-1, 1)).double() - grad).abs().max().item() / 1e-6
    print(f"loss C={C}: logits {prof['min']:.1f} .. {prof['max']:.1f}, row maxima {prof['lowest_row_max']:.1f} .. "
          f"{prof['highest_row_max']:.1f}, {prof['underflow']} underflow, {prof['subnormal']} subnormal, target p = 0 on "
          f"{prof['target_has_p0']} rows, p = 1 on {prof['target_has_p1']}, {prof['near_ties']} near ties of {count} rows "
          f"({hits} hits, nll {nll:.1f}); float32 share of the bars: nll {nll_share:.3f}, gradient {grad_share:.3f} "
          f"(folded lse: {folded:.3f})")
    assert_loss_profile(prof, C)
    assert nll_share <= WELL_POSED_SHARE and grad_share <= WELL_POSED_SHARE
    if C > 1:
        assert folded > 1.0
        # gradient rows of the two extremes: -1 / +1 on two classes and exactly 0 elsewhere; exactly 0 everywhere
        g = g32[rows]
        assert bool(((g == -1).sum(1) == 1)[(g == 1).sum(1) == 1].any())
        assert bool((g == 0).all(1).any())


# ---- SuperGAT ---------------------------------------------------------------------------------------------------------

SUPERGAT_SHAPES = [(8, 8, True), (8, 40, False), (1, 7, True)]
SUPERGAT_GRAPHS = ("random", "hub", "powerlaw")   # `powerlaw` for the late-spike property, as for GAT
# make_case keeps t = <h_j, att_l> + <h_i, att_r> near -3 on even heads and +3 on odd heads, and e = leaky_relu(t *
# sigmoid(d)) compresses the negative side by 0.2: the even heads carry 1 / 0.2 times the scale of the odd heads, so
# that both reach the same |e| (and the same float32 error of e)
SUPERGAT_SCALE_POS, SUPERGAT_SCALE_NEG = 60.0, 300.0
SUPERGAT_SEEDS = {"random": 100, "hub": 200, "powerlaw": 300}   # tests/test_gpu_supergat.py's seeds for its two graphs


SUPERGAT_SPIKE = 2.5
# chosen greedily from the graph alone: the sources whose FIRST slot lies in the last quarter of the most rows of >= 65 slots
SUPERGAT_POWERLAW_SPIKES = (416, 1453, 635, 703, 277, 770, 1121)


@functools.lru_cache(maxsize=None)
def supergat_spikes(graph_name):
    """Source nodes whose constant feature is SUPERGAT_SPIKE in place of 1. make_case pins t = <h_j, att_l> + <h_i, att_r>
    to +-3 (1 +- 0.1) and sigmoid(d) to 0.73 +- 0.05, so a row's scores have no tail: no slot lies 40 above the others
    whatever the scale. A spike source's t is +-1.5 * (2.5 + 1), some 90 above the rest of an odd head's row at scale 60.
    `hub`: two sources with one slot each in the hub row, in its first and in its last chunk, so the middle chunk's
    maximum lies below both (of the candidates, the first pair for which the heads disagree about the larger of the
    two); `powerlaw`: SUPERGAT_POWERLAW_SPIKES; `random`: none (it has no row of 65 slots)."""
    _, n = graph_of(graph_name)
    if graph_name == "random":
        return ()
    src, dst, rowptr, order = slots_of(graph_name)
    if graph_name == "powerlaw":
        return SUPERGAT_POWERLAW_SPIKES
    hub = int((rowptr[1:] - rowptr[:-1]).argmax())
    row = src[order[rowptr[hub]:rowptr[hub + 1]]]
    once = torch.bincount(row, minlength=n) == 1
    last = (row.numel() - 1) // LONG_ROW_SLOTS
    first_chunk = [int(u) for u in row[:LONG_ROW_SLOTS] if once[u] and int(u) != hub]
    last_chunk = [int(u) for u in row[last * LONG_ROW_SLOTS:] if once[u] and int(u) != hub]
    return first_chunk[0], last_chunk[2]


def supergat_case(H, C, concat, graph_name, p=0.0, lin_scale=1.0):
    """(x float64 [n, 12], reference layer): make_case's layer with att_l, att_r times the per-head scale; `lin_scale`
    multiplies the projection's weights other than the constant channel's, which spreads d = <h_i, h_j>."""
    from test_gpu_supergat import make_case
    ei, n = graph_of(graph_name)
    x, ref = make_case(H, C, concat, SUPERGAT_SEEDS[graph_name], ei, p=p)
    if x.size(0) < n:  # make_case sizes x by the largest endpoint: the hub graph's isolated nodes get rows of their own
        more = torch.randn(n - x.size(0), x.size(1), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
        more[:, 0] = 1.0
        x = torch.cat([x, more])
    x = f32_exact(x)
    x[list(supergat_spikes(graph_name)), 0] = SUPERGAT_SPIKE
    with torch.no_grad():
        for h in range(H):
            scale = SUPERGAT_SCALE_NEG if h % 2 == 0 else SUPERGAT_SCALE_POS
            ref.att_l[0, h] *= scale
            ref.att_r[0, h] *= scale
        if lin_scale != 1.0:
            keep = ref.lin.weight[::C].clone()
            ref.lin.weight.mul_(lin_scale)
            ref.lin.weight[::C] = keep
        for prm in ref.parameters():
            prm.copy_(f32_exact(prm))
    return x, ref


def supergat_formula(x, weight, att_l, att_r, bias, cot, src, dst, n, H, C, concat):
    """SuperGATConv in eval mode in the precision of the inputs: (out, [g_x, g_weight, g_att_l, g_att_r, g_bias], e)."""
    x, weight, att_l, att_r, bias = _leaves(x.dtype, x, weight, att_l, att_r, bias)
    h = (x @ weight.t()).view(n, H, C)
    hj, hi = h[src], h[dst]
    d = (hi * hj).sum(-1)
    s = ((hj * att_l).sum(-1) + (hi * att_r).sum(-1)) * torch.sigmoid(d)
    e = F.leaky_relu(s, SLOPE)
    alpha = segment_softmax(e, dst, n)
    out = torch.zeros(n, H, C, dtype=e.dtype).index_add(0, dst, alpha.unsqueeze(-1) * hj)
    out = (out.reshape(n, H * C) if concat else out.mean(1)) + bias
    (out * cot.to(e.dtype)).sum().backward()
    return out.detach(), [x.grad, weight.grad, att_l.grad, att_r.grad, bias.grad], e.detach(), s.detach(), d.detach()


SUPERGAT_NAMES = ("forward", "g_x", "g_lin.weight", "g_att_l", "g_att_r", "g_bias")


def supergat_cot(ref, n, seed):
    width = ref.H * ref.C if ref.concat else ref.C
    return torch.randn(n, width, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64)


SUPERGAT_WIDE = (8, 8, True, "random", 4.5)   # the case whose projection is scaled: d = <h_i, h_j> reaches +-30


def supergat_operands(x, ref, n, seed=1):
    return (x, ref.lin.weight.detach(), ref.att_l.detach(), ref.att_r.detach(), ref.bias.detach(),
            supergat_cot(ref, n, seed))


def assert_branch_is_sure(ref):
    """The wide case's form of assert_no_kink: s = t * sigmoid(d) comes within 1e-20 of zero where sigmoid(d) does, but
    its sign is t's as long as float32's sigmoid(d) is not 0 (d > -87), and t stays clear of zero."""
    t = (ref.s / torch.sigmoid(ref.d)).detach().abs()
    assert t.min().item() > 1e-5 * t.max().item(), (t.min().item(), t.max().item())
    assert ref.d.min().item() > -80


def check_supergat_host(H, C, concat, graph, lin_scale):
    ei, n = graph_of(graph)
    src, dst, _, _ = slots_of(graph)
    x, ref = supergat_case(H, C, concat, graph, lin_scale=lin_scale)
    ops_ = supergat_operands(x, ref, n)
    want = supergat_formula(*ops_, src, dst, n, H, C, concat)
    # the formula is the project's restatement in eval mode
    ref.eval()
    xr = x.clone().requires_grad_(True)
    out = ref(xr, ei)
    (out * ops_[-1]).sum().backward()
    theirs = (out.detach(), [xr.grad, ref.lin.weight.grad, ref.att_l.grad, ref.att_r.grad, ref.bias.grad])
    assert max(shares_of(want, theirs, SUPERGAT_NAMES).values()) < 1e-6, "this module's formula is not the restatement's"
    low = supergat_formula(*(t.float() for t in ops_), src, dst, n, H, C, concat)
    assert all(torch.isfinite(t).all() for t in [low[0]] + low[1])
    shares = shares_of(low, want, SUPERGAT_NAMES)
    prof = score_profile(want[2], graph)
    show(f"supergat ({H}, {C}, {concat}) {graph} lin x {lin_scale}", prof, shares)
    assert max(abs(prof["max_e"]), abs(prof["min_e"])) >= 100
    for name in ("underflow", "subnormal", "saturated"):
        assert PROPERTIES[name](prof), name
    assert max(shares.values()) <= WELL_POSED_SHARE, shares
    return ref, prof


@pytest.mark.parametrize("graph", SUPERGAT_GRAPHS)
@pytest.mark.parametrize("H,C,concat", SUPERGAT_SHAPES)
def test_supergat_case_is_in_range_and_well_posed(H, C, concat, graph):
    from test_gpu_supergat import assert_no_kink
    ref, _ = check_supergat_host(H, C, concat, graph, 1.0)
    assert_no_kink(ref)


def test_supergat_wide_case_saturates_sigmoid():
    H, C, concat, graph, lin_scale = SUPERGAT_WIDE
    ref, _ = check_supergat_host(H, C, concat, graph, lin_scale)
    assert_branch_is_sure(ref)
    d = ref.d.detach()
    sg = torch.sigmoid(d.float())
    print(f"d in [{d.min().item():.1f}, {d.max().item():.1f}], head mean in [{d.mean(-1).min().item():.1f}, "
          f"{d.mean(-1).max().item():.1f}]; float32 sigmoid(d) == 1 on {int((sg == 1).sum())}, < 1e-7 on {int((sg < 1e-7).sum())} "
          f"of {d.numel()}")
    assert d.min().item() <= -30 and d.max().item() >= 30
    assert int((sg == 1).sum()) > 0 and int((sg < 1e-7).sum()) > 0
    assert d.mean(-1).abs().max().item() > 20   # the link loss's softplus is linear there


def test_supergat_family_shows_every_property():
    profs = {}
    for graph in SUPERGAT_GRAPHS:
        _, n = graph_of(graph)
        src, dst, _, _ = slots_of(graph)
        for H, C, concat in SUPERGAT_SHAPES:
            x, ref = supergat_case(H, C, concat, graph)
            e = supergat_formula(*supergat_operands(x, ref, n), src, dst, n, H, C, concat)[2]
            profs[(H, C, graph)] = score_profile(e, graph)
    fam = union_profile(list(profs.values()))
    show("supergat family", fam)
    for name, holds in PROPERTIES.items():
        assert holds(fam), name
    assert any({"first", "last"} <= p["chunks"] for (H, C, g), p in profs.items() if g == "hub")


# ---- the per-edge softmax of a single head (ops.gat_edge_softmax) ------------------------------------------------------------
#
# Its bar is ABSOLUTE (1e-6 on every coefficient, tests/test_gpu_parity.py::test_gat_edge_softmax_kernel), which random
# scores of several hundred cannot meet in float32 at all: s = a_src + a_dst rounds at ulp(500) / 2 = 1.5e-5 and
# 0.2f * s at 1e-5, and a row with a near tie turns that into 4e-6 of alpha. So that the comparison is about the
# softmax and not about forming the scores, the scores lie on a grid of 1/64 and the slope is 0.25: sum and product
# are then exact in float32, and e - max is too.
EDGE_SOFTMAX_SLOPE = 0.25


@functools.lru_cache(maxsize=None)
def edge_softmax_case():
    """a_src, a_dst [n] on the hub graph: multiples of 1/64 of GAT's two scales (float64, fp32-exact)."""
    _, n = graph_of("hub")
    g = torch.Generator().manual_seed(4000)
    grid = lambda scale: torch.round(torch.randn(n, generator=g) * scale * 64).double() / 64
    return grid(GAT_SRC_SCALE), grid(GAT_DST_SCALE)


def edge_softmax_formula(a_src, a_dst):
    """(alpha, alpha_pos [E'] in CSR SLOT order, a_pos [n], row maxima [n], e [E', 1] in edge order) in the inputs' precision."""
    _, n = graph_of("hub")
    src, dst, _, order = slots_of("hub")
    s = a_src[src] + a_dst[dst]
    e = torch.where(s > 0, s, EDGE_SOFTMAX_SLOPE * s).view(-1, 1)
    alpha = O.segment_softmax(e, dst, n).view(-1)
    pos = torch.where(s > 0, alpha, torch.zeros_like(alpha))
    a_pos = torch.zeros(n, dtype=alpha.dtype).index_add(0, dst, pos)
    mx = torch.full((n,), -1e30, dtype=alpha.dtype).scatter_reduce(0, dst, e.view(-1), "amax")
    return alpha[order], pos[order], a_pos, mx, e


def test_edge_softmax_case_is_in_range_and_well_posed():
    a_src, a_dst = edge_softmax_case()
    want = edge_softmax_formula(a_src, a_dst)
    low = edge_softmax_formula(a_src.float(), a_dst.float())
    assert torch.equal(low[4].double(), want[4]) and torch.equal(low[3].double(), want[3])   # the scores are exact
    prof = score_profile(want[4], "hub")
    share = max((low[k].double() - want[k]).abs().max().item() for k in (0, 1)) / 1e-6
    show("gat_edge_softmax hub", prof, {"alpha (of 1e-6)": share, "a_pos": share_of_tolerance(low[2], want[2], FWD_TOL)})
    for name in ("overflow", "low row", "underflow", "subnormal", "saturated"):
        assert PROPERTIES[name](prof), name
    assert prof["chunks"], "the hub row's chunk maxima must lie 40 apart"
    assert share <= WELL_POSED_SHARE
