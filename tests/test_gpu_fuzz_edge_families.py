"""Seeded differential fuzz of the edge-feature, typed and gated operators merged after tests/test_gpu_fuzz_families.py:
ops.resgated_aggregate, softmax_aggregate, gine_aggregate, cgconv_aggregate, rgcn_aggregate (select and mix forms),
film_aggregate, gmm_aggregate, pna_aggregate and the bfloat16 gather (propagate_rows_bf16, propagate_bf16,
spmm_bf16_raw), each against the float64 restatement its pinned tests use (tests/test_*_host.py `aggregate` /
`operator`, oracle/ref_cpu.propagate). It is the third fuzz, in the shape of the second, whose graphs, operand layouts
and comparison it imports. What these families add to the dispatch space and the pinned tests fix at a handful of
values: a per-slot operand (e_slot / c_slot) with a leading dimension and an alignment of its own, relation-expanded
CSRs with hub plans of their own (TypedView.select, TypedView.expand_fwd), column blocking above 256 channels, and
parameter vectors the kernels read from device memory (t, mu, sigma, comp, eps). tests/test_fuzz_edge_families_host.py
replays the pinned seeds on the CPU and asserts that they reach every class.

Edges reach the restatement in the device's forward slot order (the stable grouping by target, asserted against
graph.fwd.perm), and the per-slot operand is drawn in that order, so that its gradient is compared row by row and a
tie's gradient goes to the lowest slot on both sides. The inputs are float32-exact float64 values (bfloat16-exact for the
bfloat16 gather). Bars: forward 1e-4, gradients 2e-4, times max(1, |ref|max) (test_transformer_host.FWD_TOL /
GRAD_TOL, which every one of these families' GPU tests uses; tests/test_gpu_bf16.py's TOL = 1e-4 for the gather's fp32
output); a miss falls under tests/test_gpu_fuzz.py's `_close` as it stands. A bfloat16 output must lie between the
roundings of the float64 result minus and plus the fp32 bar: it is the float64 result rounded, or its neighbour where a
rounding boundary lies within the bar.

Non-smooth points are decided from the float64 reference alone. GINE's x and e are multiples of 1 / 8, so x_j + e_p is
one exact fp32 add and relu takes the same branch on both sides (relu'(0) = 0 on both). FiLM draws
test_film_host.operator_case's grid (odd multiples for h and gamma: fmaf(gamma, h, beta) is exact and zero only at the
planted ties). PNA zeroes the cotangent of the max / min entries test_pna_host.violations reports a gap violation for and
of the var / std entries with a variance violation, leaves the latter out of the forward comparison, and redraws a case
in which more than a tenth of those blocks is zeroed. A softmax row with 256 or more copies of one edge gets a zero
cotangent (FF.duplicate_rows). Before every call the allocator's free blocks of the output's and the gradients' sizes are
filled with NaN and the results must be finite. No case is skipped."""
import random

import pytest
import torch

import test_cgconv_host as CH
import test_film_host as FH
import test_genconv_host as SH
import test_gine_host as GH
import test_gmm_host as MH
import test_gpu_fuzz as F0
import test_gpu_fuzz_families as FF
import test_pna_host as PH
import test_resgated_host as RH
import test_rgcn_host as TH
from oracle import ref_cpu as O
from test_gpu_fuzz_families import (DEGREES, NODES, T, as_kernel_sees, compare, draw_layout, f32_exact,  # noqa: F401
                                    head_width_supported, layout_geometry, make_layout, min_vec, place, place_cotangent,
                                    prescribed_graph, rewritten_edges, row_lengths, vec_by_width)
from test_gpu_transformer import poison
from test_transformer_host import FWD_TOL, GRAD_TOL

pytestmark = pytest.mark.gpu

KINDS = ["resgated", "softmax", "gine", "cgconv", "rgcn", "film", "gmm", "pna", "bf16"]
LOOPS_KEEP, LOOPS_ADD_REMAINING = FF.LOOPS_KEEP, FF.LOOPS_ADD_REMAINING
BF16_TOL = 1e-4               # tests/test_gpu_bf16.py
MAX_REDRAWS = FF.MAX_REDRAWS
CHANNELS = FF.CHANNELS
REFUSED = FF.REFUSED                                   # one launch: up to 256 channels
BLOCKED = ("gine", "film")                             # wider inputs run as column blocks of 256
BLOCKED_WIDTHS = {"gine": [260, 300, 512], "film": [258, 300]}
BLOCKED_REFUSED = [65, 67, 129, 130, 321, 386]         # 256 + 65, 256 + 130: the last block is refused
TYPED = ("rgcn", "film")
PNA_TOWER_WIDTHS = [4, 8, 12, 32, 64, 100, 128, 256]
PNA_REFUSED = [2, 6, 7, 260]                           # (F, towers): F % 4 != 0, or above 256
PNA_CAP = 0.1                                          # the largest share of zeroed entries in the max / min / var / std blocks
BF16_WIDTHS = [8, 16, 24, 40, 64, 128, 200, 256]
ANY_WIDTHS = [1, 3, 7, 8, 12, 33, 100, 260]
GMM_K, GMM_D = [1, 2, 3, 8, 25], [1, 2, 3, 8]
SUPPORT_TEXT = "pad the"                               # every refusal of these ops says what to pad


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ---- the draws -----------------------------------------------------------------------------------------------------------

def width_supported(kind, C):
    """The rule of *_supported, restated: one head of C channels on the 64 lanes of a wave; GINE and FiLM run a wider
    input as column blocks of 256, so there the last block decides."""
    if kind in BLOCKED and C > 256:
        return head_width_supported(C % 256 or 256)
    return head_width_supported(C)


def draw_width(rng, kind, refused, limit=512, extra=()):
    if refused:
        return rng.choice(BLOCKED_REFUSED if kind in BLOCKED else REFUSED)
    return rng.choice([w for w in CHANNELS + list(extra) if w <= limit])


def draw_edge_types(rng, c):
    """int64 [E], one relation per input edge. 'by_target' / 'by_source': every node owns one relation and all edges
    into it / out of it carry that, so the relation-expanded forward / transposed row of a prescribed node has exactly the
    prescribed length; 'uniform': at random. With R > 1 the last relation owns no edge."""
    g = torch.Generator().manual_seed(rng.randrange(1 << 30))
    R, n, ei = c["R"], c["n"], c["ei"]
    live = max(R - 1, 1)
    c["et_style"] = rng.choice(["by_target", "by_source", "uniform"])
    if c["et_style"] == "uniform":
        return torch.randint(0, live, (ei.size(1),), generator=g)
    of_node = torch.randint(0, live, (n,), generator=g)
    return of_node[ei[1] if c["et_style"] == "by_target" else ei[0]]


def nonempty_subset(rng, names):
    return FF.nonempty_subset(rng, names)


def draw_case(seed, kind=None):
    """Every draw of a seed, from random.Random(seed) alone: no device, no package import."""
    rng = random.Random(seed)
    kind = kind or KINDS[seed % len(KINDS)]
    c = {"seed": seed, "kind": kind, "mode": LOOPS_KEEP, "n": rng.choice(NODES)}
    n = c["n"]
    if kind == "bf16":
        c["agg"] = rng.choice(["gcn", "mean", "sum"])
        c["mode"] = LOOPS_ADD_REMAINING if c["agg"] == "gcn" else LOOPS_KEEP       # tests/test_gpu_bf16.MODE
    if rng.random() < 0.5:
        c["ei"], c["din"], c["dout"] = prescribed_graph(rng, n, c["mode"])
        c["style"] = "prescribed"
    else:
        c["ei"], c["din"], c["dout"], c["style"] = F0.make_graph(rng, n), [], [], "random"
    ei = c["ei"]
    c["E"] = ei.size(1)
    c["run"] = rng.choice(["no_grad", "eval", "eval"])
    c["cot"] = rng.choice(["dense", "stride2", "block"])
    c["vec_off"] = rng.choice([1, 2, 3]) if rng.random() < 1.0 / 3.0 else 0
    c["refused"] = rng.random() < 0.1 and kind != "bf16"
    ref = c["refused"]
    if kind == "resgated":
        c["C"] = draw_width(rng, kind, ref)
        c["mats"], c["slot_mats"], c["vecs"] = ["k", "q", "v"], [], []
    elif kind == "softmax":
        c["C"] = draw_width(rng, kind, ref)
        c["t_form"] = rng.choice(["scalar", "channel"])
        c["t_value"] = rng.choice(["zero", "negative", "range"])      # the scalar; per channel all three occur at once
        c["mats"], c["slot_mats"], c["vecs"] = ["m"], [], ["t"]
    elif kind == "gine":
        c["C"] = draw_width(rng, kind, ref, extra=BLOCKED_WIDTHS[kind] if rng.random() < 0.25 else ())
        if not ref and rng.random() < 0.15:
            c["C"] = rng.choice(BLOCKED_WIDTHS[kind])
        c["eps_form"] = rng.choice([None, "fixed", "learned"])
        c["mats"], c["slot_mats"] = ["x", "e"], ["e"]
        c["vecs"] = ["eps"] if c["eps_form"] == "learned" else []
    elif kind == "cgconv":
        c["C"] = draw_width(rng, kind, ref)
        c["aggr"] = rng.choice(["add", "mean"])
        c["with_c"], c["with_root"] = rng.random() < 0.7, rng.random() < 0.5
        c["mats"] = ["a", "b"] + (["c"] if c["with_c"] else []) + (["root"] if c["with_root"] else [])
        c["slot_mats"], c["vecs"] = (["c"] if c["with_c"] else []), []
    elif kind == "rgcn":
        c["form"] = rng.choice(["select", "mix"])
        c["R"] = rng.choice([1, 2, 3, 5, 8])
        c["B"] = rng.choice([1, 2, 4]) if c["form"] == "mix" else c["R"]
        c["refused"] = ref = ref and c["form"] == "mix"             # the select form takes every width
        c["C"] = draw_width(rng, kind, ref, limit=512 // c["B"])
        c["aggr"] = rng.choice(["mean", "add"])
        c["with_y0"] = rng.random() < 0.5
        c["et"] = draw_edge_types(rng, c)
        c["mats"], c["slot_mats"] = ["h"] + (["y0"] if c["with_y0"] else []), []
        c["vecs"] = ["comp"] if c["form"] == "mix" else []
    elif kind == "film":
        c["typed"] = rng.random() < 0.75
        c["R"] = rng.choice([1, 2, 4]) if c["typed"] else 1
        c["C"] = draw_width(rng, kind, ref)
        if not ref and rng.random() < 0.15:
            c["C"] = rng.choice(BLOCKED_WIDTHS[kind])
        c["aggr"], c["act"] = rng.choice(["mean", "add"]), rng.choice(["relu", "identity"])
        c["with_y0"] = rng.random() < 0.5
        c["et"] = draw_edge_types(rng, c)
        c["mats"], c["slot_mats"], c["vecs"] = ["h", "fb"] + (["y0"] if c["with_y0"] else []), [], []
    elif kind == "gmm":
        c["K"], c["D"] = rng.choice(GMM_K), rng.choice(GMM_D)
        c["C"] = draw_width(rng, kind, ref, limit=512 // c["K"])            # M
        if ref:
            c["K"] = 1
        c["aggr"] = rng.choice(["mean", "add"])
        c["with_y0"] = rng.random() < 0.5
        c["degree_pseudo"] = c["D"] == 2 and rng.random() < 1.0 / 3.0
        c["mats"] = ["h"] + ([] if c["degree_pseudo"] else ["e"]) + (["y0"] if c["with_y0"] else [])
        c["slot_mats"], c["vecs"] = ([] if c["degree_pseudo"] else ["e"]), ["mu", "sigma"]
    elif kind == "pna":
        names = list(PH.AGGREGATORS)
        rng.shuffle(names)
        c["aggrs"] = tuple(names[:rng.randint(1, len(names))])
        names = list(PH.SCALERS)
        rng.shuffle(names)
        c["scalers"] = tuple(names[:rng.randint(1, len(names))])
        c["F"] = rng.choice(PNA_REFUSED if ref else PNA_TOWER_WIDTHS)
        c["towers"] = rng.choice([t for t in (1, 2, 3, 4) if t * c["F"] <= 512])
        c["d"] = c["towers"] * c["F"]
        c["with_a"], c["with_c"] = rng.random() < 0.6, rng.random() < 0.6
        c["mats"] = (["a"] if c["with_a"] else []) + ["b"] + (["c"] if c["with_c"] else [])
        c["slot_mats"], c["vecs"] = (["c"] if c["with_c"] else []), []
    elif kind == "bf16":
        c["op"] = rng.choice(["rows", "any", "raw"])
        c["d"] = rng.choice(ANY_WIDTHS if c["op"] == "any" else BF16_WIDTHS + ([264] if c["op"] == "raw" else []))
        c["addend"] = c["op"] == "rows" and rng.random() < 0.5
        c["bias"] = c["op"] != "any" and rng.random() < 0.5
        c["transposed"] = c["op"] == "raw" and rng.random() < 0.5
        c["out_dtype"] = "bf16" if c["op"] == "raw" and rng.random() < 0.5 else "fp32"
        c["mats"], c["slot_mats"] = ["x"] + (["y"] if c["op"] == "raw" and rng.random() < 0.5 else []), []
        c["vecs"] = ["bias"] if c["bias"] else []
        if c["op"] == "raw":
            c["run"] = "no_grad"                                     # spmm_bf16_raw has no autograd
    c["layouts"] = {m: draw_layout(rng) for m in c["mats"]}
    c["req"] = nonempty_subset(rng, c["mats"] + c["vecs"])
    if c.get("t_form") and rng.random() < 0.3 and "t" in c["req"] and len(c["req"]) > 1:
        c["req"].remove("t")
    c["desc"] = " ".join(f"{k}={v}" for k, v in c.items() if k not in ("ei", "et", "mats", "vecs", "slot_mats"))
    return c


def slot_order(c):
    """(perm, src, dst[, et]) in forward CSR slot order: the input edges stably grouped by target (LOOPS_KEEP)."""
    src, dst = c["ei"][0], c["ei"][1]
    perm = torch.argsort(dst, stable=True)
    return perm, src[perm], dst[perm]


def mat_shape(c, m):
    kind, n, E = c["kind"], c["n"], c["E"]
    if kind == "bf16":
        return (n, 2 * c["d"] if c["addend"] and m == "x" else c["d"])
    rows = E if m in c["slot_mats"] else n
    if kind == "pna":
        return (rows, c["d"])
    C = c["C"]
    if kind == "cgconv":
        return (rows, C if m == "root" else 2 * C)
    if kind == "rgcn":
        return (rows, c["B"] * C if m == "h" else C)
    if kind == "film":
        return (rows, {"h": c["R"] * C, "fb": 2 * c["R"] * C, "y0": C}[m])
    if kind == "gmm":
        return (rows, {"h": c["K"] * C, "e": c["D"], "y0": C}[m])
    return (rows, C)


def out_shape(c):
    kind, n = c["kind"], c["n"]
    if kind == "pna":
        return (n, c["towers"] * len(c["scalers"]) * len(c["aggrs"]) * c["F"])
    return (n, c["d"] if kind == "bf16" else c["C"])


# ---- data ------------------------------------------------------------------------------------------------------------------

def bf16_exact(shape, gen):
    return torch.randn(shape, generator=gen).to(torch.bfloat16).double()


def make_data(c, data_seed):
    """name -> float64 tensor with float32-exact values, plus 'cot' (and the PNA masks). Per-slot operands are drawn in
    forward slot order."""
    g = torch.Generator().manual_seed(data_seed)
    kind, n, E = c["kind"], c["n"], c["E"]
    d = {}
    if kind in ("resgated", "cgconv", "pna"):
        d = {m: f32_exact(mat_shape(c, m), g) for m in c["mats"]}
    elif kind == "softmax":
        C = c["C"]
        lo, hi = -2.0, 4.0                                   # test_genconv_host.set_parameters' t_range
        t = (torch.rand(C if c["t_form"] == "channel" else 1, generator=g) * (hi - lo) + lo).double()
        if c["t_form"] == "channel":
            t[0] = 0.0
            t[-1] = -t[-1].abs() - 0.25
        elif c["t_value"] != "range":
            t[0] = 0.0 if c["t_value"] == "zero" else -t[0].abs() - 0.25
        d = {"m": f32_exact((n, C), g), "t": t.float().double()}
    elif kind == "gine":
        d = {m: FH._grid(mat_shape(c, m), g) for m in c["mats"]}
        d["eps"] = f32_exact((1,), g, 0.5)
    elif kind == "rgcn":
        d = {m: f32_exact(mat_shape(c, m), g) for m in c["mats"]}
        d["comp"] = f32_exact((c["R"], c["B"]), g)
    elif kind == "film":
        R, C = c["R"], c["C"]
        rows, gamma, beta = FH._grid((n, R, C), g, odd=True), FH._grid((n, R, C), g, odd=True), FH._grid((n, R, C), g)
        src, dst, et = c["ei"][0], c["ei"][1], c["et"]
        k, ch = FH.tie_positions(E, C)
        if k.numel():
            gamma[dst[k], et[k], ch], beta[dst[k], et[k], ch], rows[src[k], et[k], ch] = 2.0, -1.0, 0.5
        d = {"h": rows.reshape(n, R * C), "fb": torch.cat([beta, gamma], dim=2).reshape(n, R * 2 * C),
             "y0": FH._grid((n, C), g)}
    elif kind == "gmm":
        K, D = c["K"], c["D"]
        d = {"h": f32_exact((n, K * c["C"]), g), "y0": f32_exact((n, c["C"]), g), "mu": MH.unit_coords((K, D), g),
             "sigma": MH.spread_sigma((K, D), g)}
        perm = slot_order(c)[0]
        d["e"] = MH.degree_pseudo(c["ei"], n).double()[perm] if c["degree_pseudo"] else MH.unit_coords((E, D), g)
    elif kind == "bf16":
        x = bf16_exact((n, c["d"]), g)
        d = {"x": torch.cat([x, f32_exact((n, c["d"]), g)], dim=1) if c["addend"] else x,
             "y": f32_exact((n, c["d"]), g), "bias": f32_exact((c["d"],), g, 0.5),
             "raw": f32_exact((n, c["d"]), g, 3.0)}                # ops.to_bf16_rows against .to(torch.bfloat16)
    d["cot"] = bf16_exact(out_shape(c), g) if kind == "bf16" else f32_exact(out_shape(c), g)
    if kind == "softmax":
        d["cot"][FF.duplicate_rows(dict(c, kind="transformer"))] = 0
    if kind == "pna" and not c["refused"]:
        _, src, dst = slot_order(c)
        u = d["b"][src] + (d["c"] if c["with_c"] else 0.0)
        gap, var = PH.violations(u, src, dst, n)
        zero = pna_mask(c, gap, var)
        d["cot"][zero] = 0
        d["band"] = pna_mask(c, torch.zeros_like(gap), var)
        blocks = pna_mask(c, torch.ones_like(gap), torch.ones_like(var))
        d["share"] = float(zero.sum()) / max(float(blocks.sum()), 1.0)
    return d


def pna_mask(c, gap, var):
    """bool mask in the output's layout [n, T, S, A, F]: `gap` [n, d] on the max / min blocks, `var` on var / std."""
    n, Tn, S, F = c["n"], c["towers"], len(c["scalers"]), c["F"]
    per = [gap if a in ("max", "min") else (var if a in ("var", "std") else torch.zeros_like(gap)) for a in c["aggrs"]]
    m = torch.stack([p.view(n, Tn, F) for p in per], dim=2)             # [n, T, A, F]
    return m[:, :, None].expand(n, Tn, S, len(per), F).reshape(n, -1).clone()


# ---- the restatements --------------------------------------------------------------------------------------------------

def pna_averages(c):
    """(avg_lin, avg_log) float32 [2]: the graph's own (ops.degree_averages), or test_pna_host.FIXED_AVG on a graph
    without edges, whose own averages are 0."""
    return PH.averages_of(c["ei"], c["n"]) if c["E"] else PH.FIXED_AVG.clone()


def bf16_edges(c, dtype):
    """(edge list after the loops mode's rewrite, weight per edge or None) of the gather's operator P, as
    tests/test_gpu_bf16.py's fixture makes them."""
    n = c["n"]
    if c["agg"] == "gcn":
        return O.gcn_norm(c["ei"], None, n, dtype=dtype)
    w = None
    if c["agg"] == "mean":
        w = (1.0 / torch.bincount(c["ei"][1], minlength=n).clamp(min=1).to(dtype))[c["ei"][1]]
    return c["ei"], w


def restate(c, L, dtype):
    """The output from the leaves L (name -> tensor of `dtype`), through the host files' own restatements."""
    kind, n = c["kind"], c["n"]
    if kind == "bf16":
        ei, w = bf16_edges(c, dtype)
        x = L["x"][:, :c["d"]]
        out = O.propagate(ei.flip(0) if c["transposed"] else ei, x, n, w, "add")
        if c["addend"]:
            out = out + L["x"][:, c["d"]:]
        if "y" in L:
            out = out + L["y"]
        return out + L["bias"] if c["bias"] else out
    perm, src, dst = slot_order(c)
    if c.get("edge_order") == "given":   # the host test: the edge list as given, the per-slot rows carried back to it
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(perm.numel())
        src, dst = c["ei"][0], c["ei"][1]
        L = {k: (v[inv] if k in c["slot_mats"] else v) for k, v in L.items()}
    if kind == "resgated":
        return RH.aggregate(L["k"], L["q"], L["v"], n, src, dst)
    if kind == "softmax":
        return SH.aggregate(L["m"], L["t"], n, src, dst)[0]
    if kind == "gine":
        eps = {None: None, "fixed": c["data"]["eps"].to(dtype), "learned": L.get("eps")}[c["eps_form"]]
        return GH.aggregate(L["x"], L["e"], n, src, dst, eps)
    if kind == "cgconv":
        return CH.aggregate(L["a"], L["b"], L.get("c"), n, src, dst, c["aggr"], L.get("root"))
    et = None
    if kind in TYPED:
        et = c["et"] if c.get("edge_order") == "given" else c["et"][perm]
    if kind == "rgcn":
        rows = TH.select_rows(L["h"], c["R"]) if c["form"] == "select" else TH.mix_rows(L["h"], L["comp"])
        out = TH.aggregate(rows, n, src, dst, et, c["aggr"])
        return out + L["y0"] if c["with_y0"] else out
    if kind == "film":
        rows, beta, gamma = FH.film_rows(L["h"], L["fb"], c["R"])
        out = FH.aggregate(rows, beta, gamma, n, src, dst, et, c["aggr"], c["act"])
        return out + L["y0"] if c["with_y0"] else out
    if kind == "gmm":
        e = L["e"] if "e" in L else c["data"]["e"].to(dtype)[inv if c.get("edge_order") == "given" else slice(None)]
        out = MH.aggregate(L["h"], e, L["mu"], L["sigma"], n, src, dst, c["aggr"])
        return out + L["y0"] if c["with_y0"] else out
    if kind == "pna":
        return PH.operator(L.get("a"), L["b"], L.get("c"), n, src, dst, c["aggrs"], c["scalers"], pna_averages(c),
                           c["F"])[0].to(dtype)
    raise ValueError(kind)


def reference(c, data, dtype=torch.float64):
    """name -> tensor: 'out' and 'g_<leaf>' for EVERY leaf of the case (None where the output does not depend on it),
    under the case's cotangent."""
    c["data"] = data
    L = {k: data[k].to(dtype).clone().requires_grad_(True) for k in c["mats"] + c["vecs"]}
    out = restate(c, L, dtype)
    total = (out * data["cot"].to(dtype)).sum()
    names = list(L)
    grads = torch.autograd.grad(total, [L[k] for k in names], allow_unused=True) if total.requires_grad else [None] * len(names)
    want = {"out": out.detach()}
    for k, g in zip(names, grads):
        want["g_" + k] = g
    return want


def well_posed(c, data, want):
    """From the float64 reference alone. PNA: the zeroed share of the max / min / var / std blocks within PNA_CAP."""
    return data.get("share", 0.0) <= PNA_CAP


def posed_data(c):
    """(data, float64 reference, redraws used): the case's data, its seed advanced until the case is well-posed. The
    shape, the graph and the options stay. A refused width has no reference."""
    for r in range(MAX_REDRAWS + 1):
        data = make_data(c, c["seed"] * 16 + r)
        want = None if c["refused"] else reference(c, data)
        if well_posed(c, data, want):
            return data, want, r
    raise AssertionError(f"{c['desc']}: ill-posed after {MAX_REDRAWS} redraws of the data")


def masked(c, data, t):
    """The output without PNA's variance band (compared nowhere: its cotangent is 0)."""
    if "band" not in data:
        return t
    t = t.clone()
    t[data["band"]] = 0
    return t


# ---- the device side ---------------------------------------------------------------------------------------------------

def place_vector(t, off, dev, requires_grad):
    """A parameter vector as the op is handed it: its own allocation, or (off > 0) a slice `off` floats into a flat
    buffer, the way tests/test_fuzz_families_host.test_parameters_off_the_grid_are_copied_too builds one. Returns
    (operand, leaf, leaf.grad -> (gradient in t's shape, gradient of the slack))."""
    if not off:
        leaf = t.float().to(dev).requires_grad_(requires_grad)
        return leaf, leaf, lambda g: (g, None)
    k = t.numel()
    base = torch.zeros(k + 4, device=dev)
    base[off:off + k] = t.float().reshape(-1).to(dev)
    base.requires_grad_(requires_grad)
    return base[off:off + k].view(t.shape), base, lambda g: (g[off:off + k].view(t.shape), torch.cat([g[:off], g[off + k:]]))


def device_forward(c, D, graph, ops):
    """The op under test on the device operands D."""
    kind = c["kind"]
    if kind == "resgated":
        return ops.resgated_aggregate(D["k"], D["q"], D["v"], graph)
    if kind == "softmax":
        return ops.softmax_aggregate(D["m"], D["t"], graph)
    if kind == "gine":
        return ops.gine_aggregate(D["x"], D["e"], graph, D.get("eps"))
    if kind == "cgconv":
        return ops.cgconv_aggregate(D["a"], D["b"], D.get("c"), graph, c["C"], c["aggr"], D.get("root"))
    if kind == "rgcn":
        return ops.rgcn_aggregate(D["h"], graph, D["et"], c["R"], D.get("comp"), c["aggr"], D.get("y0"))
    if kind == "film":
        return ops.film_aggregate(D["h"], D["fb"], graph, D["et"] if c["typed"] else None, c["R"], c["aggr"], c["act"],
                                  D.get("y0"))
    if kind == "gmm":
        e = ops.degree_pseudo(graph) if c["degree_pseudo"] else D["e"]
        return ops.gmm_aggregate(D["h"], e, D["mu"], D["sigma"], graph, c["aggr"], D.get("y0"))
    if kind == "pna":
        return ops.pna_aggregate(D.get("a"), D["b"], D.get("c"), graph, list(c["aggrs"]), list(c["scalers"]), D["avg"],
                                 c["F"])
    if c["op"] == "rows":
        return ops.propagate_rows_bf16(D["x"], graph, c["agg"], c["d"], D.get("bias"))
    if c["op"] == "any":
        return ops.propagate_bf16(D["x"], graph, c["agg"])
    csr = graph.bwd if c["transposed"] else graph.fwd
    w, rs = ops._kind_weights(graph, c["agg"], c["transposed"])
    xb = ops.to_bf16_rows(D["x"])
    assert torch.equal(xb.cpu().view(torch.int16), D["x"].detach().cpu().contiguous().to(torch.bfloat16).view(torch.int16))
    raw = ops.to_bf16_rows(D["raw"])
    assert torch.equal(raw.cpu().view(torch.int16), D["raw"].cpu().contiguous().to(torch.bfloat16).view(torch.int16)), \
        "to_bf16_rows differs from .to(torch.bfloat16)"
    return ops.spmm_bf16_raw(csr, w, rs, xb, y=D.get("y"), a=1.0, b=1.0, bias=D.get("bias"),
                             out_dtype=torch.bfloat16 if c["out_dtype"] == "bf16" else torch.float32)


def supported_on_device(c, ops):
    kind, C = c["kind"], c.get("C")
    if kind == "pna":
        # rgbx_pna_supported speaks of ONE launch (d <= 256); the op cuts a wider d at tower boundaries (pna_blocks)
        F, d = c["F"], c["d"]
        rule = F >= 4 and F % 4 == 0 and d % F == 0 and F <= 256
        widths = [(t1 - t0) * F for t0, t1 in pna_blocks(d, F)] if rule else [d]
        return all(ops.pna_supported(w, F) for w in widths), rule
    if kind == "gmm":
        return ops.gmm_supported(c["K"], C, c["D"]), 1 <= c["K"] <= 64 and 1 <= c["D"] <= 8 and head_width_supported(C)
    if kind == "rgcn":
        if c["form"] == "select":
            return True, True
        return ops.rgcn_mix_supported(c["B"], C), 1 <= c["B"] <= 64 and head_width_supported(C)
    if kind in BLOCKED:
        pred = ops.gine_supported if kind == "gine" else ops.film_supported
        return pred(C % 256 or 256) if C > 256 else pred(C), width_supported(kind, C)
    pred = {"resgated": ops.resgated_supported, "softmax": ops.softmax_aggregate_supported,
            "cgconv": ops.cgconv_supported}[kind]
    return pred(C), head_width_supported(C)


def pna_blocks(d, F):
    """[(t0, t1)]: the towers of every launch of ops.pna_aggregate, as many as fit into 256 channels (restated)."""
    per = max(256 // F, 1)
    return [(t0, min(t0 + per, d // F)) for t0 in range(0, d // F, per)]


def bf16_round(t):
    return t.float().to(torch.bfloat16).double()


def run_edge_family_case(dev, seed, kind=None):
    from rgb_experiment_amd import graph as G
    from rgb_experiment_amd import ops
    assert G.LONG_ROW_SLOTS == T and (G.LOOPS_KEEP, G.LOOPS_ADD_REMAINING) == (LOOPS_KEEP, LOOPS_ADD_REMAINING)
    c = draw_case(seed, kind)
    kind, n, desc = c["kind"], c["n"], c["desc"]
    try:
        data, want, redraws = posed_data(c)
        desc += f" redraws={redraws}"
        G.clear_cache()
        graph = G.get_graph(c["ei"].to(dev), n, c["mode"])
        lengths = row_lengths(c["ei"], n, c["mode"])
        assert torch.equal((graph.fwd.rowptr[1:] - graph.fwd.rowptr[:-1]).cpu().long(), lengths[0]), "forward row lengths"
        assert torch.equal((graph.bwd.rowptr[1:] - graph.bwd.rowptr[:-1]).cpu().long(), lengths[1]), "transposed row lengths"
        if c["mode"] == LOOPS_KEEP:
            assert graph.fwd.nnz == c["E"]
            assert torch.equal(graph.fwd.perm[:c["E"]].cpu().long(), slot_order(c)[0]), "forward slot order"
        if kind != "bf16":
            got_s, rule = supported_on_device(c, ops)
            assert bool(got_s) == bool(rule) == (not c["refused"]), ("supported", got_s, rule)
        grad_on = c["run"] != "no_grad"
        D, leaves = {}, {}
        for m in c["mats"]:
            D[m], leaf, split = place(data[m], c["layouts"][m], dev, grad_on and m in c["req"])
            leaves[m] = (leaf, split)
        for v in c["vecs"]:
            D[v], leaf, split = place_vector(data[v], c["vec_off"], dev, grad_on and v in c["req"])
            leaves[v] = (leaf, split)
        if kind == "gine" and c["eps_form"] == "fixed":
            D["eps"] = place_vector(data["eps"], c["vec_off"], dev, False)[0]
        if kind in TYPED:
            D["et"] = c["et"].to(dev)
        if kind == "pna":
            D["avg"] = ops.degree_averages(graph) if c["E"] else PH.FIXED_AVG.to(dev)
            host = pna_averages(c)
            assert float((D["avg"].cpu() - host).abs().max()) <= 1e-6 * float(host.abs().max()), "degree_averages"
        if kind == "bf16":
            D["raw"] = place(data["raw"], c["layouts"]["x"], dev, False)[0]
        shapes = {out_shape(c)} | {tuple(data[m].shape) for m in c["mats"]}
        poison(dev, *[s for s in shapes if s[0] * s[1] > 0])
        if c["refused"]:
            with pytest.raises(RuntimeError, match=SUPPORT_TEXT):
                device_forward(c, D, graph, ops)
            return
        with torch.set_grad_enabled(grad_on):
            out_d = device_forward(c, D, graph, ops)
        cache = {}

        def want32(name):
            if "r" not in cache:
                cache["r"] = reference(c, data, torch.float32)
            return lambda: masked(c, data, cache["r"][name]) if name == "out" else cache["r"][name]

        assert tuple(out_d.shape) == out_shape(c), ("out", tuple(out_d.shape))
        assert bool(torch.isfinite(out_d.float()).all()), "out: a row was left unwritten"
        ref_out = masked(c, data, want["out"])
        if kind == "bf16" and c["out_dtype"] == "bf16":
            assert out_d.dtype == torch.bfloat16
            bar = BF16_TOL * max(1.0, ref_out.abs().max().item() if ref_out.numel() else 1.0)
            got = out_d.cpu().double()
            lo, hi = bf16_round(ref_out - bar), bf16_round(ref_out + bar)
            assert bool(((got >= lo) & (got <= hi)).all()), ("out (bfloat16)", float((got - bf16_round(ref_out)).abs().max()))
        else:
            assert out_d.dtype == torch.float32
            compare(c, "out", masked(c, data, out_d.detach().cpu().double()), ref_out, BF16_TOL if kind == "bf16" else FWD_TOL,
                    want32("out"))
        if not grad_on:
            assert not out_d.requires_grad
            return
        if not out_d.requires_grad:
            assert all(want["g_" + k] is None for k in c["req"]), "the output takes no gradient"
            return
        out_d.backward(place_cotangent(data["cot"], c["cot"], dev))
        for k, (leaf, split) in leaves.items():
            ref_g = want["g_" + k]
            if k not in c["req"] or ref_g is None:
                # (a graph without edges: the gradient of a per-slot operand is [0, d], and of nothing the maximum is none)
                assert leaf.grad is None or (ref_g is None and not (leaf.grad.numel() and float(leaf.grad.abs().max()))), \
                    (k, "unasked gradient")
                continue
            assert leaf.grad is not None, (k, "no gradient")
            g, slack = split(leaf.grad)
            if slack is not None and slack.numel():
                assert float(slack.abs().max()) == 0.0, (k, "gradient outside the operand's columns")
            compare(c, "g_" + k, g, ref_g, GRAD_TOL, want32("g_" + k))
    except AssertionError as exc:
        raise AssertionError(f"{desc}: {exc}") from exc
    except RuntimeError as exc:
        raise RuntimeError(f"{desc}: {exc}") from exc


# Seeds in the suite: blocks of 9 consecutive seeds, one case of every kind each. Blocks 0 .. 39 as they come; 42, 44, 50, 55,
# 70 and 110 are the first later blocks with the eight classes those miss (a transposed row of T + 1 slots for cgconv and
# the width 128 for bf16; a transposed and a relation-expanded transposed row of T slots for film; pna's a without a
# gradient beside b or c with one; G = 1 for softmax; a relation-expanded forward row of T slots for rgcn; G = 1 for
# rgcn's mix form). tests/test_fuzz_edge_families_host.py asserts that these blocks reach every class for every kind and
# prints the table; thousands of seeds beyond them are tools/fuzz_soak.py --edge-families'
# (profiles/edge_families_fuzz_soak.txt).
PINNED_BLOCKS = list(range(40)) + [42, 44, 50, 55, 70, 110]


def pinned_seeds():
    n = len(KINDS)
    return [b * n + i for b in PINNED_BLOCKS for i in range(n)] + [s for s in SOAK_FOUND if s // n not in PINNED_BLOCKS]


@pytest.mark.parametrize("block", PINNED_BLOCKS)
def test_edge_families_against_their_restatements_on_random_shapes(dev, block):
    for seed in range(block * len(KINDS), (block + 1) * len(KINDS)):
        run_edge_family_case(dev, seed)


SOAK_FOUND = [8, 5650, 3148]


@pytest.mark.parametrize("seed", SOAK_FOUND)
def test_seeds_the_soak_found(dev, seed):
    """What the runs of this fuzz turned up (CHANGELOG, profiles/edge_families_fuzz_soak.txt); the first also runs
    inside its block. 8 (bf16, ops.spmm_bf16_raw over the transposed CSR, the bias a slice one float into a flat buffer,
    the addend y a column block): rgbx_spmm_csr_bf16 reads y and bias four floats at a time and refused the call ("y / out / bias
    must be 16-byte aligned with ld % 4 == 0"), and ops.propagate_rows_bf16 hands it a bias through .contiguous() and the
    addend half of an offset h as it is; spmm_bf16_raw now puts y through ops._rows_on_grid and the bias through
    ops._vec_on_grid, as the fp32 families do. 5650 (pna, var and std under inverse_linear, two nodes, one of them with a
    single in-edge): g_b 5.8e-4 off a gradient that is 0 everywhere. The backward forms B (u_p - mean_u) as B u_p - B mean_u;
    on a row of one slot u_p = mean_u and the true term is 0, but B = 2 g lin / 1 = 3109 there and the two halves cancel at
    that size. The float32 restatement, which subtracts first, is 6e-7 off, so this was the op's arithmetic and not the
    case: _PNAAggregate.backward now sets B to 0 on rows of fewer than two slots, which is exact. 3148 (pna, max alone, a
    graph without edges, c_slot with a gradient): the restatement's output does not depend on c, the device returns the
    [0, d] gradient, and this file's own check for a zero unasked gradient took the maximum of nothing; mended here."""
    run_edge_family_case(dev, seed)
