"""Seeded differential fuzz of the operators added after tests/test_gpu_fuzz.py's kinds: ops.gatv2_attend,
transformer_attend, supergat_attend, faconv, gru_step, propagate_max / propagate_min, propagate_multi and the edge-weighted
propagate_gcn_edge_weight / APPNP / SGConv, each against the float64 restatement the pinned tests of its family use
(tests/test_*_host.py, oracle/ref_cpu.py). The pinned tests fix a handful of shapes on two or three graphs; this walks the
dispatch space between them: every lane layout of csrc/attn_common.h (vector width by C and by the operands' alignment,
ragged last head chunks, idle lanes), rows of exactly 0, 1, 64, 65, T, T + 1, 2T + 1, 3T + 7 slots in the forward and the
transposed CSR (T = graph.LONG_ROW_SLOTS), graphs of 1, 2 and 3 nodes, operands that are column blocks or offset views,
non-contiguous cotangents, and the options in combination. tests/test_fuzz_families_host.py replays the pinned seeds'
draws on the CPU and asserts that they reach every one of these classes.

The inputs are float32-exact float64 values, so both sides hold the same numbers. Every case checks the output and every
gradient element by element at the bars of the family's pinned tests: forward 1e-4, gradients 2e-4, times
max(1, |ref|max); the extremum forward (and the max / min blocks of the multi-aggregation) must be EQUAL; the weighted
family keeps tests/test_gpu_edge_weight.py's 1e-4 for both. A case the draw made badly conditioned (thousands of duplicate
edges into one row, p_drop = 0.9 on a row of one slot) falls under tests/test_gpu_fuzz.py's `_close` rule as it stands:
within the bar, OR within 16 times what the float32 run of the same restatement on the CPU is off from the float64 one.

Training mode feeds the restatement the device's own decisions (ops.*_random_choices). Non-smooth points are decided from
the reference alone: GATv2's s = xl + xr is one fp32 add of exact values (tests/test_gpu_gatv2.py); SuperGAT's parameters
follow tests/test_gpu_supergat.make_case's construction and the data seed is advanced (at most 8 times) until
assert_no_kink's criterion holds on the float64 reference; std's band (test_multi_aggr_host.std_band) is left out of the
forward comparison and gets a zero cotangent; a row of the softmax families with 256 or more copies of one edge gets a
zero cotangent (duplicate_rows). No case is skipped."""
import math
import random

import pytest
import torch

import test_gpu_fuzz as F0
from oracle import ref_cpu as O
from test_extremum_host import host_csr, ref_extremum
from test_fagcn_host import RefFAConv
from test_gatv2_host import RefGATv2Conv
from test_ggnn_host import RefGatedGraphConv
from test_multi_aggr_host import ref_stat, std_band
from test_supergat_host import RefSuperGATConv
from test_transformer_host import attend as transformer_attend_ref

pytestmark = pytest.mark.gpu

KINDS = ["gatv2", "transformer", "supergat", "faconv", "gru", "extremum", "multi", "weighted"]
ATTENTION = ("gatv2", "transformer", "supergat", "faconv")
FWD_TOL, GRAD_TOL = 1e-4, 2e-4
WEIGHTED_TOL = 1e-4           # tests/test_gpu_edge_weight.py: forward and gradients
OWN_FACTOR = 16.0             # test_gpu_fuzz._close
T = 1024                      # graph.LONG_ROW_SLOTS (asserted where the package is imported)
LOOPS_KEEP, LOOPS_ADD_REMAINING, LOOPS_REMOVE_ADD = 0, 1, 2
LOOPS = {"gatv2": LOOPS_REMOVE_ADD, "supergat": LOOPS_REMOVE_ADD, "faconv": LOOPS_ADD_REMAINING,
         "weighted": LOOPS_ADD_REMAINING, "transformer": LOOPS_KEEP, "gru": LOOPS_KEEP, "extremum": LOOPS_KEEP,
         "multi": LOOPS_KEEP}
NODES = [1, 2, 3, 31, 33, 64, 100, 257, 700]
DEGREES = [0, 1, 2, 63, 64, 65, 128, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 7]
HEADS = [1, 2, 3, 4, 5, 6, 8, 9, 12]
CHANNELS = [1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 20, 24, 31, 32, 33, 40, 48, 63, 64, 66, 96, 100, 126, 128, 132, 192, 252, 256]
REFUSED = [65, 67, 129, 130, 258, 260]
WIDTHS = [1, 3, 4, 7, 8, 12, 33, 64, 100, 128, 256, 260]            # extremum, multi, weighted
GRU_WIDTHS = [1, 3, 4, 7, 8, 12, 16, 30, 32, 33, 40, 63, 64, 65, 96, 128]
STATS = ("sum", "mean", "var", "std", "max", "min")
P_DROP = [0.1, 0.5, 0.9]
MAX_REDRAWS = 8
SLOPE = 0.2
KINK = 1e-5                   # test_gpu_supergat.assert_no_kink: smallest |s| above KINK * max |s|
SOFTMAX = ("gatv2", "transformer", "supergat")
DUP_LIMIT = 256               # copies of one edge in a row from which the row's cotangent is zeroed (duplicate_rows)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


# ---- the layout of csrc/attn_common.h, restated ----------------------------------------------------------------------

def pow2ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def head_width_supported(C):
    return C > 0 and (C <= 64 or (C % 2 == 0 and C <= 128) or (C % 4 == 0 and C <= 256))


def vec_by_width(C):
    return 4 if C % 4 == 0 else (2 if C % 2 == 0 else 1)


def min_vec(C):
    """The narrowest vector width at which 64 lanes still cover a head of C channels."""
    return 1 if C <= 64 else (2 if C <= 128 else 4)


def make_layout(H, C, vec):
    """(LPH, HPC, G) of make_layout."""
    lph = pow2ceil((C + vec - 1) // vec)
    hpc = min(H, 64 // lph)
    return lph, hpc, pow2ceil(hpc * lph)


# ---- graphs ------------------------------------------------------------------------------------------------------------

def prescribed_graph(rng, n, mode):
    """A few targets with exact in-degrees and a few sources with exact out-degrees out of DEGREES, counted AFTER the loops
    mode's rewrite (a mode that removes self-loops and adds one per node leaves d - 1 other slots in a row of d, and no row
    of 0); sources are random, so duplicates occur. The other edges avoid those targets and sources. Returns
    (edge_index, [in-degrees], [out-degrees])."""
    g = torch.Generator().manual_seed(rng.randrange(1 << 30))
    rewritten = mode != LOOPS_KEEP
    nodes = list(range(n))
    rng.shuffle(nodes)
    k_t = min(rng.choice([1, 2, 3, 4]), n)
    k_s = min(rng.choice([0, 1, 2, 3]), n - k_t)
    tg, sc = nodes[:k_t], nodes[k_t:k_t + k_s]
    parts = []
    e = rng.choice([0, n // 2 + 1, 3 * n])
    if e:
        base = torch.randint(0, n, (2, e), generator=g)
        ok = ~torch.isin(base[1], torch.tensor(tg)) & ~torch.isin(base[0], torch.tensor(sc, dtype=torch.int64))
        parts.append(base[:, ok])

    def star(centre, others_not, d):
        want = max(d - 1, 0) if rewritten else d
        pool = [v for v in range(n) if v not in others_not and not (rewritten and v == centre)]
        if not pool:
            pool = [v for v in range(n) if not (rewritten and v == centre)]
        if not pool or want == 0:
            return None
        return torch.tensor(pool)[torch.randint(0, len(pool), (want,), generator=g)]

    din, dout = [], []
    for t in tg:
        d = rng.choice(DEGREES)
        din.append(d)
        other = star(t, sc, d)
        if other is not None:
            parts.append(torch.stack([other, torch.full_like(other, t)]))
    for s in sc:
        d = rng.choice(DEGREES)
        dout.append(d)
        other = star(s, tg, d)
        if other is not None:
            parts.append(torch.stack([torch.full_like(other, s), other]))
    ei = torch.cat(parts, dim=1) if parts else torch.zeros((2, 0), dtype=torch.int64)
    return ei[:, torch.randperm(ei.size(1), generator=g)], din, dout


def rewritten_edges(ei, n, mode):
    """(src, dst) after the loops mode's rewrite; the order is that of the families' host restatements."""
    if mode == LOOPS_KEEP:
        return ei[0], ei[1]
    keep = ei[0] != ei[1]
    loops = torch.arange(n, dtype=ei.dtype)
    return torch.cat([ei[0][keep], loops]), torch.cat([ei[1][keep], loops])


def duplicate_rows(c):
    """bool [n]: the targets whose row holds DUP_LIMIT or more copies of one edge, for the softmax families. From the
    graph alone. A float32 accumulator that adds one value m times rounds the same way on every step, so the row's
    aggregate drifts by up to m 2^-25 of itself instead of sqrt(m) 2^-24 (any order of summation that keeps runs of equal
    terms does, the kernels' and the CPU's alike). The backward of these families takes the softmax Jacobian's
    D_i = <gout_i, out_i> from that aggregate, a dot product over C <= 256 channels of N(0, 1) values of size about
    sqrt(C) <= 16, and subtracts it from <gout_i, x_j> of the same size: the drift enters the gradients as up to
    16 m 2^-25, which reaches the gradients' bar of 2e-4 at m = 419. Rows from 256 copies on therefore get a zero
    cotangent (their forward is compared like every other row's; their backward runs, on zeros), as std's band does:
    seed 4168 (profiles/families_fuzz_soak.txt) is what such a row does otherwise."""
    n = c["n"]
    if c["kind"] not in SOFTMAX:
        return torch.zeros(n, dtype=torch.bool)
    src, dst = rewritten_edges(c["ei"], n, c["mode"])
    pairs, counts = torch.unique(dst * n + src, return_counts=True)
    rows = torch.zeros(n, dtype=torch.bool)
    rows[(pairs[counts >= DUP_LIMIT] // n)] = True
    return rows


def row_lengths(ei, n, mode):
    """Row lengths of the rewritten forward CSR (by target) and of its transpose (by source)."""
    src, dst = rewritten_edges(ei, n, mode)
    return torch.bincount(dst, minlength=n), torch.bincount(src, minlength=n)


# ---- operand layouts ---------------------------------------------------------------------------------------------------

def draw_layout(rng):
    """fresh | a column block of one wider matrix (leading dimension 2F, 3F or F + pad) | a view that starts k floats in."""
    kind = rng.choice(["fresh", "fresh", "block", "block", "offset"])
    if kind == "block":
        wide = rng.choice(["2F", "3F", "pad"])
        return ("block", wide, rng.choice([1, 2, 3, 4, 6, 8]) if wide == "pad" else 0, rng.randrange(3))
    if kind == "offset":
        return ("offset", rng.choice([1, 2, 3]))
    return ("fresh",)


def layout_geometry(spec, n, F):
    """(total floats of the base buffer, first float of the operand, leading dimension)."""
    if spec[0] == "block":
        _, wide, pad, which = spec
        ld = {"2F": 2 * F, "3F": 3 * F, "pad": F + pad}[wide]
        c0 = (which % (ld // F)) * F if wide != "pad" else (0, pad, pad // 2)[which]
        return n * ld, c0, ld
    if spec[0] == "offset":
        return n * F + 4, spec[1], F
    return n * F, 0, F


def as_kernel_sees(spec, n, F, copies):
    """(offset of the first float from a 16-byte boundary, leading dimension) of the operand the kernel is handed.
    `copies`: the op calls .contiguous() on it — a non-contiguous view arrives as a fresh matrix; an offset view and a
    one-row block ARE contiguous and arrive as they are. A one-row matrix has leading dimension F (_lib.mat)."""
    _, c0, ld = layout_geometry(spec, n, F)
    if n <= 1:
        ld = F
    if copies and ld != F:
        return 0, F
    return c0, ld


def place(t, spec, dev, requires_grad):
    """float64 [n, F] -> (operand view on the device, leaf that takes the gradient, function leaf.grad -> [n, F] gradient
    and the gradient of the slack, which must stay zero)."""
    n, F = t.shape
    total, c0, ld = layout_geometry(spec, n, F)
    if spec[0] == "fresh":
        leaf = t.float().to(dev).requires_grad_(requires_grad)
        return leaf, leaf, lambda g: (g, None)
    base = torch.randn(total, generator=torch.Generator().manual_seed(total)).to(dev)
    if spec[0] == "block":
        base.view(n, ld)[:, c0:c0 + F] = t.float().to(dev)
        base.requires_grad_(requires_grad)
        view = base.view(n, ld)[:, c0:c0 + F]

        def split(g):
            g = g.view(n, ld)
            slack = torch.cat([g[:, :c0], g[:, c0 + F:]], dim=1)
            return g[:, c0:c0 + F], slack
        return view, base, split
    base[c0:c0 + n * F] = t.float().to(dev).reshape(-1)
    base.requires_grad_(requires_grad)
    view = base[c0:c0 + n * F].view(n, F)
    return view, base, lambda g: (g[c0:c0 + n * F].view(n, F), torch.cat([g[:c0], g[c0 + n * F:]]))


def place_cotangent(t, how, dev):
    """A cotangent the backward cannot take as it is: the op's .contiguous() copy runs."""
    c = t.float().to(dev)
    if how == "dense" or c.dim() != 2:
        return c
    n, F = c.shape
    if how == "stride2":
        wide = torch.zeros((n, 2 * F), device=dev)
        wide[:, ::2] = c
        return wide[:, ::2]
    wide = torch.zeros((n, F + 3), device=dev)
    wide[:, 3:] = c
    return wide[:, 3:]


# ---- the draws -----------------------------------------------------------------------------------------------------------

def f32_exact(shape, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).double()


def nonempty_subset(rng, names):
    while True:
        pick = [a for a in names if rng.random() < 0.6]
        if pick:
            return pick


def draw_case(seed, kind=None):
    """Every draw of a seed, from random.Random(seed) alone: no device, no package import."""
    rng = random.Random(seed)
    kind = kind or KINDS[seed % len(KINDS)]
    mode = LOOPS[kind]
    c = {"seed": seed, "kind": kind, "mode": mode, "n": rng.choice(NODES)}
    n = c["n"]
    if rng.random() < 0.5:
        c["ei"], c["din"], c["dout"] = prescribed_graph(rng, n, mode)
        c["style"] = "prescribed"
    else:
        c["ei"], c["din"], c["dout"], c["style"] = F0.make_graph(rng, n), [], [], "random"
    c["run"] = rng.choice(["no_grad", "eval", "eval", "train", "train"])
    c["p_drop"] = rng.choice(P_DROP) if c["run"] == "train" else 0.0
    c["cot"] = rng.choice(["dense", "stride2", "block"])
    if kind in ATTENTION:
        c["refused"] = rng.random() < 0.1
        C = rng.choice(REFUSED if c["refused"] else CHANNELS)
        H = 1 if kind == "faconv" else rng.choice([h for h in HEADS if h * C <= 512])
        c["H"], c["C"] = H, C
        c["bias"] = rng.random() < 0.6
        c["concat"] = rng.random() < 0.7
    if kind == "gatv2":
        c["mats"], c["vecs"] = ["xl", "xr"], ["att"] + (["bias"] if c["bias"] else [])
    elif kind == "transformer":
        c["mats"], c["vecs"] = ["q", "k", "v"], []
        c["scale"] = rng.choice([1.0 / math.sqrt(c["C"]), 1.0 / c["C"], 0.37])
    elif kind == "supergat":
        c["mats"], c["vecs"] = ["h"], ["att_l", "att_r"] + (["bias"] if c["bias"] else [])
        c["pos_ratio"] = rng.choice([1.0, 0.8])
    elif kind == "faconv":
        c["mats"], c["vecs"] = ["x", "x0"], ["att_l", "att_r"]
        c["eps"] = rng.choice([0.0, 0.1, 0.3])
        c["form"] = rng.choice([None, "fused", "composed"])
    elif kind == "gru":
        C = rng.choice(GRU_WIDTHS)
        Cp = (C + 3) // 4 * 4 if rng.random() < 0.6 else (C + 7) // 8 * 8
        fused_ok = Cp % 8 == 0 and Cp <= 64          # ops.gru_step_supported (asserted on the device)
        c["C"], c["Cp"] = C, Cp
        c["form"] = rng.choice([None, "general"] + (["fused", "composed"] if fused_ok else []))
        c["bias"] = rng.random() < 0.7
        c["mats"] = ["x"]
        c["vecs"] = ["weight", "w_ih", "w_hh"] + (["b_ih", "b_hh"] if c["bias"] else [])
    elif kind == "extremum":
        c["d"] = rng.choice(WIDTHS)
        c["op"] = rng.choice(["max", "min"])
        c["bag_of_words"] = rng.random() < 1.0 / 3.0
        c["mats"], c["vecs"] = ["x"], []
    elif kind == "multi":
        c["d"] = rng.choice(WIDTHS)
        names = list(STATS)
        rng.shuffle(names)
        c["aggrs"] = tuple(names[:rng.randint(1, len(names))])
        c["mats"], c["vecs"] = ["x"], []
    elif kind == "weighted":
        c["d"] = rng.choice(WIDTHS)
        c["op"] = rng.choice(["gcn", "appnp", "sgc"])
        c["K"], c["alpha"] = rng.choice([1, 2, 5]), rng.choice([0.0, 0.1, 0.5])
        c["d_out"] = rng.choice([1, 4, 7, 16, 40])
        c["bias"] = rng.random() < 0.6
        a = rng.randrange(n)  # two self-loops on one node (test_two_self_loops_known_answer: the last one's weight wins)
        c["ei"] = torch.cat([c["ei"], torch.tensor([[a, a], [a, a]])], dim=1)
        c["mats"] = ["x"]
        c["vecs"] = {"gcn": ["ew"] + (["bias"] if c["bias"] else []), "appnp": [],
                     "sgc": ["W"] + (["bias"] if c["bias"] else [])}[c["op"]]
    if kind not in ATTENTION:
        c["run"] = "no_grad" if c["run"] == "no_grad" else "eval"
        c["p_drop"] = 0.0
    c["layouts"] = {m: draw_layout(rng) for m in c["mats"]}
    c["req"] = nonempty_subset(rng, c["mats"] + c["vecs"])
    c["E"] = c["ei"].size(1)
    c["desc"] = " ".join(f"{k}={v}" for k, v in c.items() if k not in ("ei", "mats", "vecs"))
    return c


def feature_width(c):
    if c["kind"] in ATTENTION:
        return c["H"] * c["C"]
    return c["C"] if c["kind"] == "gru" else c["d"]


def layout_class(c):
    """The lane layout the attention kernels run a case at: (vec, lowered by an operand, LPH, HPC, G, chunks, heads in the
    last chunk), or None for a refused width. pick_vec takes the widest of 4, 2 that divides C and that every operand's
    pointer and leading dimension allow; an operand off the grid of min_vec(C) is copied by the op first. FAConv's
    kernels take the width from C alone (an operand off that grid is copied) and have one head."""
    kind, H, C = c["kind"], c["H"], c["C"]
    if not head_width_supported(C):
        return None
    F = H * C
    vec = vec_by_width(C)
    if kind != "faconv":
        for m in c["mats"]:
            off, ld = as_kernel_sees(c["layouts"][m], c["n"], F, copies=kind == "supergat")
            if off % min_vec(C) or ld % min_vec(C):
                continue  # copied: aligned
            while vec > 1 and (off % vec or ld % vec):
                vec //= 2
    lph, hpc, G = make_layout(H, C, vec)
    chunks = (H + hpc - 1) // hpc
    return {"vec": vec, "lowered": vec < vec_by_width(C), "LPH": lph, "HPC": hpc, "G": G, "chunks": chunks,
            "last": H - (chunks - 1) * hpc}


# ---- data ------------------------------------------------------------------------------------------------------------------

def make_data(c, data_seed):
    """name -> float64 tensor with float32-exact values, plus 'cot' (and 'band' for std)."""
    g = torch.Generator().manual_seed(data_seed)
    kind, n = c["kind"], c["n"]
    d = {}
    if kind == "gatv2":
        H, C = c["H"], c["C"]
        d = {"xl": f32_exact((n, H * C), g), "xr": f32_exact((n, H * C), g), "att": f32_exact((1, H, C), g, C ** -0.5),
             "bias": f32_exact((H * C,), g)}
    elif kind == "transformer":
        F = c["H"] * c["C"]
        d = {"q": f32_exact((n, F), g), "k": f32_exact((n, F), g), "v": f32_exact((n, F), g)}
    elif kind == "supergat":
        # test_gpu_supergat.make_case at the operator's input: channel 0 of every head is the constant 1 and both
        # attention vectors carry -1.5 (even heads) / +1.5 (odd heads) on it, so t = <h_j, att_l> + <h_i, att_r> stays
        # near -3 / +3; the other channels of h have standard deviation 0.5 / C^(1/4), the attention vectors 0.1
        H, C = c["H"], c["C"]
        h = torch.randn(n, H, C, generator=g) * (0.5 / C ** 0.25)
        h[:, :, 0] = 1.0
        att_l, att_r = torch.randn(1, H, C, generator=g) * 0.1, torch.randn(1, H, C, generator=g) * 0.1
        for hd in range(H):
            sign = -1.0 if hd % 2 == 0 else 1.0
            att_l[0, hd, 0] += 1.5 * sign
            att_r[0, hd, 0] += 1.5 * sign
        d = {"h": h.reshape(n, H * C).double(), "att_l": att_l.double(), "att_r": att_r.double(),
             "bias": f32_exact((H * C,), g, 0.4)}
    elif kind == "faconv":
        C = c["C"]
        d = {"x": f32_exact((n, C), g), "x0": f32_exact((n, C), g), "att_l": f32_exact((1, C), g, C ** -0.5),
             "att_r": f32_exact((1, C), g, C ** -0.5)}
    elif kind == "gru":
        C = c["C"]
        u = lambda *shape: ((torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(C)).double()
        d = {"x": f32_exact((n, C), g), "weight": u(C, C), "w_ih": u(3 * C, C), "w_hh": u(3 * C, C),
             "b_ih": f32_exact((3 * C,), g, 0.5), "b_hh": f32_exact((3 * C,), g, 0.5)}
    elif kind in ("extremum", "multi"):
        x = torch.randn(n, c["d"], generator=g)
        if c.get("bag_of_words"):
            x = (torch.rand(n, c["d"], generator=g) < 0.3).float()
        d = {"x": x.double()}
    elif kind == "weighted":
        d = {"x": f32_exact((n, c["d"]), g), "ew": (torch.rand(c["E"], generator=g) * 3.75 + 0.25).double(),
             "W": f32_exact((c["d_out"], c["d"]), g, c["d"] ** -0.5)}
        d["bias"] = f32_exact((c["d_out"] if c["op"] == "sgc" else c["d"],), g, 0.5)
    d["cot"] = f32_exact(out_shape(c), g)
    d["cot"][duplicate_rows(c)] = 0
    if kind == "multi" and "std" in c["aggrs"]:
        rowptr, col = host_csr(c["ei"], n)
        d["band"] = std_band(rowptr, col, d["x"])
        s, w = c["aggrs"].index("std"), c["d"]
        d["cot"][:, s * w:(s + 1) * w][d["band"]] = 0
    return d


def out_shape(c):
    kind, n = c["kind"], c["n"]
    if kind in ("gatv2", "transformer", "supergat"):
        return (n, c["H"] * c["C"]) if c["concat"] else (n, c["C"])
    if kind == "multi":
        return (n, len(c["aggrs"]) * c["d"])
    if kind == "weighted" and c["op"] == "sgc":
        return (n, c["d_out"])
    return (n, feature_width(c))


# ---- the restatements --------------------------------------------------------------------------------------------------
# reference(): the suite's float64 restatement. generic(): the same formulas in the dtype of the inputs, for the float32 run
# of a badly conditioned case (the suite's restatement classes allocate in float64); the host test asserts that both
# agree in float64.

def _set(module, name, tensor):
    """A restatement's parameter replaced by the leaf itself, so that the leaf's gradient is the reference's."""
    delattr(module, name)
    setattr(module, name, tensor)


def _merge_heads(out, c):
    n, H, C = c["n"], c["H"], c["C"]
    return out.reshape(n, H * C) if c["concat"] else out.reshape(n, H, C).mean(1)


def _edge_softmax(e, msg, dst, n, keep, p):
    H = e.size(1)
    mx = torch.full((n, H), -1e30, dtype=e.dtype).scatter_reduce(0, dst.view(-1, 1).expand(-1, H), e.detach(), "amax")
    ex = torch.exp(e - mx[dst])
    den = torch.zeros(n, H, dtype=e.dtype).index_add(0, dst, ex)
    alpha = ex / (den[dst] + 1e-16)
    if keep is not None:
        alpha = alpha * keep.to(e.dtype) / (1.0 - p)
    return torch.zeros((n,) + tuple(msg.shape[1:]), dtype=e.dtype).index_add(0, dst, alpha.unsqueeze(-1) * msg)


def _supergat_loss(d, h, choices):
    pos = d[choices["pos"]].mean(-1)
    u, v = choices["neg"][0][choices["valid"]], choices["neg"][1][choices["valid"]]
    neg = (h[u] * h[v]).sum(-1).mean(-1)
    logits = torch.cat([pos, neg])
    if logits.numel() == 0:  # the op divides the summed terms by max(count, 1)
        return logits.sum()
    labels = torch.cat([torch.ones_like(pos), torch.zeros_like(neg)])
    return torch.nn.functional.binary_cross_entropy_with_logits(logits, labels)


def restate(c, L, choices, suite):
    """{'out': ..., ['att_loss': ...]} from the leaves L (name -> tensor that requires grad, float64 or float32).
    `suite`: through the suite's restatement classes (float64 only), else through the generic formulas."""
    kind, n = c["kind"], c["n"]
    dtype = L[c["mats"][0]].dtype
    train = c["run"] == "train"
    p = c["p_drop"]
    if choices is None:
        src, dst = rewritten_edges(c["ei"], n, c["mode"])
    else:
        src, dst = choices["src"], choices["dst"]
    res = {}
    if kind == "gatv2":
        H, C = c["H"], c["C"]
        keep = choices["keep"] if train else None
        xl, xr = L["xl"].view(n, H, C), L["xr"].view(n, H, C)
        if suite:
            ref = RefGATv2Conv(1, C, heads=H, negative_slope=SLOPE, dropout=p)
            _set(ref, "att", L["att"])  # the leaf itself, so that its gradient is the reference's
            out = ref.attend(xl, xr, n, src, dst, keep)
        else:
            s = xl[src] + xr[dst]
            e = (L["att"] * torch.nn.functional.leaky_relu(s, SLOPE)).sum(-1)
            out = _edge_softmax(e, xl[src], dst, n, keep, p)
        out = out.reshape(n, H * C)
        res["out"] = _merge_heads(out + L["bias"] if c["bias"] else out, c)
    elif kind == "transformer":
        H, C = c["H"], c["C"]
        keep = choices["keep"] if train else None
        out, _ = transformer_attend_ref(L["q"].view(n, H, C), L["k"].view(n, H, C), L["v"].view(n, H, C), n, src, dst,
                                        c["scale"], keep, p)
        res["out"] = _merge_heads(out, c)
    elif kind == "supergat":
        H, C = c["H"], c["C"]
        if suite:
            ref = RefSuperGATConv(H * C, C, heads=H, concat=True, negative_slope=SLOPE, dropout=p)
            with torch.no_grad():
                ref.lin.weight.copy_(torch.eye(H * C, dtype=torch.float64))  # h = x, exactly
            _set(ref, "att_l", L["att_l"])
            _set(ref, "att_r", L["att_r"])
            _set(ref, "bias", L["bias"] if c["bias"] else torch.zeros(H * C, dtype=torch.float64))
            ref.train(train)
            if train and int(choices["pos"].sum()) + int(choices["valid"].sum()) == 0:
                # no loss term at all: the op divides the summed terms by max(count, 1), so its loss is 0; the
                # restatement's mean of nothing is not a number, so it is given every positive and its loss a weight of 0
                out = ref(L["h"], c["ei"], dict(choices, pos=torch.ones_like(choices["pos"])))
                res["att_loss"] = ref.att_loss * 0.0
            else:
                out = ref(L["h"], c["ei"], choices)
                if train:
                    res["att_loss"] = ref.att_loss
            res["s"] = ref.s.detach()
        else:
            h = L["h"].view(n, H, C)
            hj, hi = h[src], h[dst]
            dd = (hi * hj).sum(-1)
            s = ((hj * L["att_l"]).sum(-1) + (hi * L["att_r"]).sum(-1)) * torch.sigmoid(dd)
            e = torch.nn.functional.leaky_relu(s, SLOPE)
            out = _edge_softmax(e, hj, dst, n, choices["drop"] if train else None, p).reshape(n, H * C)
            if c["bias"]:
                out = out + L["bias"]
            if train:
                res["att_loss"] = _supergat_loss(dd, h, choices)
            res["s"] = s.detach()
        res["out"] = _merge_heads(out, c)
    elif kind == "faconv":
        C = c["C"]
        if suite:
            ref = RefFAConv(C, eps=c["eps"], dropout=p)
            _set(ref.att_l, "weight", L["att_l"])
            _set(ref.att_r, "weight", L["att_r"])
            ref.train(train)
            res["out"] = ref(L["x"], L["x0"], c["ei"], choices)
        else:
            deg = torch.zeros(n, dtype=dtype).index_add(0, dst, torch.ones(dst.numel(), dtype=dtype))
            dis = deg.pow(-0.5)
            al, ar = (L["x"] @ L["att_l"].t()).view(-1), (L["x"] @ L["att_r"].t()).view(-1)
            k = choices["keep"].to(dtype) / (1.0 - p) if train else torch.ones(src.numel(), dtype=dtype)
            coef = k * torch.tanh(al[src] + ar[dst]) * dis[src] * dis[dst]
            out = torch.zeros_like(L["x"]).index_add(0, dst, coef.unsqueeze(-1) * L["x"][src])
            res["out"] = out + c["eps"] * L["x0"] if c["eps"] != 0.0 else out
    elif kind == "gru":
        C = c["C"]
        ref = RefGatedGraphConv(C, 1).to(dtype)
        zero = torch.zeros(3 * C, dtype=dtype)
        _set(ref, "weight", L["weight"].view(1, C, C))
        _set(ref.rnn, "weight_ih", L["w_ih"])
        _set(ref.rnn, "weight_hh", L["w_hh"])
        _set(ref.rnn, "bias_ih", L["b_ih"] if c["bias"] else zero)
        _set(ref.rnn, "bias_hh", L["b_hh"] if c["bias"] else zero)
        res["out"] = ref(L["x"], c["ei"])
    elif kind == "extremum":
        rowptr, col = c.get("csr") or host_csr(c["ei"], n)
        res["out"] = ref_extremum(rowptr, col, L["x"], c["op"])[0]
    elif kind == "multi":
        rowptr, col = c.get("csr") or host_csr(c["ei"], n)
        res["out"] = torch.cat([ref_stat(rowptr, col, L["x"], a) for a in c["aggrs"]], dim=1)
    elif kind == "weighted":
        ew = L["ew"] if "ew" in L else c["data"]["ew"].to(dtype)
        # of several self-loops on one node the LAST one's weight is the loop's (add_remaining_self_loops): the others
        # do not enter the result, so their gradient is zero. The oracle writes them with one indexed assignment, whose
        # autograd hands the gradient to every written value, the overwritten ones included: they are taken out first
        loop = c["ei"][0] == c["ei"][1]
        last = torch.full((n,), -1, dtype=torch.int64).scatter_reduce(0, c["ei"][0][loop], torch.arange(c["E"])[loop], "amax")
        live = ~loop | (last[c["ei"][0]] == torch.arange(c["E"]))
        ei2, w = O.gcn_norm(c["ei"][:, live], ew[live], n, dtype=dtype)
        if c["op"] == "gcn":
            out = O.propagate(ei2, L["x"], n, w)
            res["out"] = out + L["bias"] if c["bias"] else out
        elif c["op"] == "appnp":
            z = L["x"]
            for _ in range(c["K"]):
                z = (1 - c["alpha"]) * O.propagate(ei2, z, n, w) + c["alpha"] * L["x"]
            res["out"] = z
        else:
            hh = L["x"]
            for _ in range(c["K"]):
                hh = O.propagate(ei2, hh, n, w)
            out = hh @ L["W"].t()
            res["out"] = out + L["bias"] if c["bias"] else out
    return res


def reference(c, data, choices, dtype=torch.float64, suite=None):
    """name -> tensor: 'out', 'att_loss' where there is one, and 'g_<leaf>' for EVERY leaf of the case (None where the
    output does not depend on it), under the case's cotangent."""
    suite = dtype == torch.float64 if suite is None else suite
    c["data"] = data
    L = {k: data[k].to(dtype).clone().requires_grad_(True) for k in c["mats"] + c["vecs"]}
    res = restate(c, L, choices, suite)
    total = (res["out"] * data["cot"].to(dtype)).sum()
    if "att_loss" in res:
        total = total + 4 * res["att_loss"]
    names = list(L)
    grads = torch.autograd.grad(total, [L[k] for k in names], allow_unused=True) if total.requires_grad else [None] * len(names)
    want = {"out": res["out"].detach()}
    if "att_loss" in res:
        want["att_loss"] = res["att_loss"].detach()
    if "s" in res:
        want["s"] = res["s"]
    for k, g in zip(names, grads):
        want["g_" + k] = g
    return want


def well_posed(c, want):
    """From the float64 reference alone. SuperGAT: assert_no_kink's criterion on the pre-activations."""
    if c["kind"] == "supergat" and want["s"].numel():
        s = want["s"].abs()
        return s.min().item() > KINK * s.max().item()
    return True


def posed_data(c):
    """(data, eval-mode float64 reference, redraws used): the case's data, its seed advanced until the case is well-posed.
    The shape, the graph and the options stay."""
    for r in range(MAX_REDRAWS + 1):
        data = make_data(c, c["seed"] * 16 + r)
        ev = dict(c, run="eval" if c["run"] == "train" else c["run"], p_drop=0.0)
        want = reference(ev, data, None)
        if well_posed(c, want):
            return data, want, r
    raise AssertionError(f"{c['desc']}: ill-posed after {MAX_REDRAWS} redraws of the data")


def synthetic_choices(c, seed):
    """Random decisions in the shapes ops.*_random_choices returns them, for the CPU replay of a training-mode case."""
    g = torch.Generator().manual_seed(seed)
    n = c["n"]
    src, dst = rewritten_edges(c["ei"], n, c["mode"])
    order = torch.argsort(dst, stable=True)
    src, dst = src[order], dst[order]
    E, H = src.numel(), c.get("H", 1)
    keep = torch.rand(E, H, generator=g) >= c["p_drop"]
    ch = {"src": src, "dst": dst, "keep": keep[:, 0] if c["kind"] == "faconv" else keep}
    if c["kind"] == "supergat":
        n_neg = int(0.5 * c["pos_ratio"] * E)
        ch.update(drop=keep, pos=torch.rand(E, generator=g) < c["pos_ratio"],
                  neg=torch.randint(0, n, (2, n_neg), generator=g), valid=torch.rand(n_neg, generator=g) < 0.9)
    return ch


# ---- comparison ----------------------------------------------------------------------------------------------------------

def bars(c):
    return (WEIGHTED_TOL, WEIGHTED_TOL) if c["kind"] == "weighted" else (FWD_TOL, GRAD_TOL)


def exact_columns(c):
    """Column mask of the output that must be EQUAL (no rounding): the extremum forward, the max / min blocks."""
    if c["kind"] == "extremum":
        return torch.ones(c["d"], dtype=torch.bool)
    if c["kind"] == "multi":
        return torch.tensor([a in ("max", "min") for a in c["aggrs"]]).repeat_interleave(c["d"])
    return None


def compare(c, name, got, want64, tol, want32):
    """test_gpu_fuzz._close as it stands: within tol x max(1, |ref|max), or within OWN_FACTOR x the float32 restatement's
    own distance from the float64 one; `want32` is a function, run only when the first bar is missed."""
    got = got.detach().cpu().double()
    assert got.shape == want64.shape, (name, tuple(got.shape), tuple(want64.shape))
    if not want64.numel():
        return
    assert bool(torch.isfinite(got).all()), (name, "not finite")
    err = (got - want64).abs().max().item()
    if err < tol * max(1.0, want64.abs().max().item()):
        return
    F0._close(name, got, want64, want32(), scale_floor=1.0, rel=tol, own_factor=OWN_FACTOR)


def masked(c, data, t):
    """The output without std's band (compared nowhere: its cotangent is 0)."""
    if "band" not in data:
        return t
    s, w = c["aggrs"].index("std"), c["d"]
    t = t.clone()
    t[:, s * w:(s + 1) * w][data["band"]] = 0
    return t


# ---- the device side ---------------------------------------------------------------------------------------------------

def device_forward(c, D, graph, record, ops):
    """{'out': ..., ['att_loss': ...]} of the op under test on the device operands D."""
    kind, n = c["kind"], c["n"]
    train, p = c["run"] == "train", c["p_drop"]
    res = {}
    if kind == "gatv2":
        out = ops.gatv2_attend(D["xl"], D["xr"], D["att"], graph, c["H"], c["C"], SLOPE, bias=D.get("bias"), training=train,
                               p_drop=p, record=record)
    elif kind == "transformer":
        out = ops.transformer_attend(D["q"], D["k"], D["v"], graph, c["H"], c["C"], c["scale"], training=train, p_drop=p,
                                     record=record)
    elif kind == "supergat":
        out, loss = ops.supergat_attend(D["h"], D["att_l"], D["att_r"], graph, c["H"], c["C"], SLOPE, bias=D.get("bias"),
                                        training=train, p_drop=p, pos_ratio=c["pos_ratio"], neg_ratio=0.5, record=record)
        if train:
            res["att_loss"] = loss
    elif kind == "faconv":
        out = ops.faconv(D["x"], D["x0"], D["att_l"], D["att_r"], graph, eps=c["eps"], training=train, p_drop=p,
                         form=c["form"], record=record)
    elif kind == "gru":
        C, Cp = c["C"], c["Cp"]
        weff, wroot, b = ops.gru_operands(D["weight"], D["w_ih"], D["w_hh"], D.get("b_ih"), D.get("b_hh"), Cp)
        x = D["x"] if Cp == C else torch.nn.functional.pad(D["x"], (0, Cp - C))
        out = ops.gru_step(x, graph, weff, wroot, b, form=c["form"])
        out = out if Cp == C else out[:, :C]
    elif kind == "extremum":
        out = (ops.propagate_max if c["op"] == "max" else ops.propagate_min)(D["x"], graph)
    elif kind == "multi":
        out = ops.propagate_multi(D["x"], graph, list(c["aggrs"]))
    elif kind == "weighted":
        from rgb_experiment_amd import nn as RN
        if c["op"] == "gcn":
            out = ops.propagate_gcn_edge_weight(D["x"], D["ew"], graph, D.get("bias"))
        elif c["op"] == "appnp":
            out = RN.APPNP(c["K"], c["alpha"])(D["x"], c["ei_dev"], c["ew_dev"])
        else:
            conv = RN.SGConv(c["d"], c["d_out"], K=c["K"], bias=c["bias"]).to(D["x"].device)
            conv.lin.weight = D["W_param"]
            if c["bias"]:
                conv.lin.bias = D["bias_param"]
            out = conv(D["x"], c["ei_dev"], c["ew_dev"])
    if kind in ("gatv2", "transformer", "supergat") and not c["concat"]:
        out = out.view(n, c["H"], c["C"]).mean(1)
    res["out"] = out
    return res


def refusal(c, D, graph, ops):
    """A refused head width: the documented error, and the predicate agrees. FAConv computes it in the composed form."""
    kind, H, C = c["kind"], c["H"], c["C"]
    supported = {"gatv2": lambda: ops.gatv2_supported(H, C), "transformer": lambda: ops.transformer_supported(H, C),
                 "supergat": lambda: ops.supergat_supported(H, C), "faconv": lambda: ops.faconv_supported(C)}[kind]()
    assert supported == head_width_supported(C), ("supported", supported)
    if supported:
        return False
    if kind == "faconv":
        assert ops.faconv_form(C) == "composed"
        if c["form"] == "fused":
            with pytest.raises(RuntimeError, match="composed"):
                device_forward(c, D, graph, {}, ops)
            c["form"] = None
        return False  # the composed form runs and is compared like any other case
    with pytest.raises(RuntimeError, match="pad the head width"):
        device_forward(c, D, graph, {}, ops)
    return True


def run_family_case(dev, seed, kind=None):
    from rgb_experiment_amd import graph as G
    from rgb_experiment_amd import ops
    assert G.LONG_ROW_SLOTS == T and (G.LOOPS_KEEP, G.LOOPS_ADD_REMAINING, G.LOOPS_REMOVE_ADD) == (0, 1, 2)
    c = draw_case(seed, kind)
    kind, n, desc = c["kind"], c["n"], c["desc"]
    try:
        data, _, redraws = posed_data(c)
        desc += f" redraws={redraws}"
        G.clear_cache()
        c["ei_dev"] = c["ei"].to(dev)
        ew_leaf = None
        if kind == "weighted":
            ew_leaf = data["ew"].float().to(dev).requires_grad_(c["op"] == "gcn" and "ew" in c["req"] and c["run"] != "no_grad")
            c["ew_dev"] = ew_leaf
            graph = G.get_graph(c["ei_dev"], n, c["mode"], ew_leaf)
        else:
            graph = G.get_graph(c["ei_dev"], n, c["mode"])
        lengths = row_lengths(c["ei"], n, c["mode"])
        assert torch.equal((graph.fwd.rowptr[1:] - graph.fwd.rowptr[:-1]).cpu().long(), lengths[0]), "forward row lengths"
        assert torch.equal((graph.bwd.rowptr[1:] - graph.bwd.rowptr[:-1]).cpu().long(), lengths[1]), "transposed row lengths"
        if kind in ("extremum", "multi"):  # ties go to the lowest slot of the device's own CSR, as in the pinned tests
            c["csr"] = (graph.fwd.rowptr.cpu().long(), graph.fwd.col[:graph.fwd.nnz].cpu().long())
        if kind == "gru":
            assert ops.gru_step_supported(c["Cp"]) == (c["Cp"] % 8 == 0 and c["Cp"] <= 64)
        grad_on = c["run"] != "no_grad"
        D, leaves = {}, {}
        for m in c["mats"]:
            D[m], leaf, split = place(data[m], c["layouts"][m], dev, grad_on and m in c["req"])
            leaves[m] = (leaf, split)
        for v in c["vecs"]:
            t = ew_leaf if v == "ew" else data[v].float().to(dev).requires_grad_(grad_on and v in c["req"])
            D[v] = t
            leaves[v] = (t, lambda g: (g, None))
        if kind == "weighted" and c["op"] == "sgc":
            D["W_param"] = torch.nn.Parameter(D["W"].detach(), requires_grad=D["W"].requires_grad)
            leaves["W"] = (D["W_param"], lambda g: (g, None))
            if c["bias"]:
                D["bias_param"] = torch.nn.Parameter(D["bias"].detach(), requires_grad=D["bias"].requires_grad)
                leaves["bias"] = (D["bias_param"], lambda g: (g, None))
        if kind in ATTENTION and refusal(c, D, graph, ops):
            return
        record = {}
        torch.manual_seed(seed)
        with torch.set_grad_enabled(grad_on):
            got = device_forward(c, D, graph, record, ops)
        choices = None
        if c["run"] == "train":
            torch.cuda.synchronize()
            fetch = {"gatv2": lambda: ops.gatv2_random_choices(record, graph, c["H"]),
                     "transformer": lambda: ops.transformer_random_choices(record, graph, c["H"]),
                     "supergat": lambda: ops.supergat_random_choices(record, graph, c["H"]),
                     "faconv": lambda: ops.faconv_random_choices(record, graph)}[kind]
            choices = {k: v.cpu() for k, v in fetch().items()}
        want = reference(c, data, choices)
        cache = {}

        def want32(name):
            if "r" not in cache:
                cache["r"] = reference(c, data, choices, torch.float32)
            return lambda: masked(c, data, cache["r"][name]) if name == "out" else cache["r"][name]

        fwd_tol, grad_tol = bars(c)
        out, ref_out = masked(c, data, got["out"].detach().cpu().double()), masked(c, data, want["out"])
        exact = exact_columns(c)
        if exact is not None and bool(exact.any()):
            assert torch.equal(out[:, exact], ref_out[:, exact]), "out: the extremum columns must be equal"
        compare(c, "out", out, ref_out, fwd_tol, want32("out"))
        if "att_loss" in want:
            compare(c, "att_loss", got["att_loss"], want["att_loss"], fwd_tol, want32("att_loss"))
        if not grad_on:
            assert not got["out"].requires_grad
            return
        outs, cots = [got["out"]], [place_cotangent(data["cot"], c["cot"], dev)]
        if "att_loss" in got and got["att_loss"].requires_grad:
            outs.append(got["att_loss"])
            cots.append(torch.tensor(4.0, device=dev))
        if not got["out"].requires_grad:
            assert all(want["g_" + k] is None for k in c["req"]), "the output takes no gradient"
            return
        torch.autograd.backward(outs, cots)
        for k, (leaf, split) in leaves.items():
            ref_g = want["g_" + k]
            if k not in c["req"] or ref_g is None:
                assert leaf.grad is None or (ref_g is None and float(leaf.grad.abs().max()) == 0.0), (k, "unasked gradient")
                continue
            assert leaf.grad is not None, (k, "no gradient")
            g, slack = split(leaf.grad)
            if slack is not None and slack.numel():
                assert float(slack.abs().max()) == 0.0, (k, "gradient outside the operand's columns")
            compare(c, "g_" + k, g, ref_g, grad_tol, want32("g_" + k))
    except AssertionError as exc:
        raise AssertionError(f"{desc}: {exc}") from exc
    except RuntimeError as exc:
        raise RuntimeError(f"{desc}: {exc}") from exc


# Seeds in the suite: blocks of 8 consecutive seeds, one case of every kind each. Blocks 0 .. 39 as they come; 42, 43, 58,
# 109 and 237 are the first later blocks with the five classes those miss (SuperGAT with an operand copied to fit a wave,
# a forward row of T + 1 slots for GATv2 and for FAConv, one lane per neighbour row for SuperGAT and for TransformerConv).
# tests/test_fuzz_families_host.py asserts that these blocks reach every layout class, row length, graph size and option
# value for every kind; thousands of seeds beyond them are tools/fuzz_soak.py --families' (profiles/families_fuzz_soak.txt).
PINNED_BLOCKS = list(range(40)) + [42, 43, 58, 109, 237]


def pinned_seeds():
    return [b * 8 + i for b in PINNED_BLOCKS for i in range(8)] + [s for s in SOAK_FOUND if s // 8 not in PINNED_BLOCKS]


@pytest.mark.parametrize("block", PINNED_BLOCKS)
def test_new_families_against_their_restatements_on_random_shapes(dev, block):
    for seed in range(block * 8, block * 8 + 8):
        run_family_case(dev, seed)


SOAK_FOUND = [0, 25, 338, 51, 15, 2291, 4168, 1804]


@pytest.mark.parametrize("seed", SOAK_FOUND)
def test_seeds_the_soak_found(dev, seed):
    """What the runs of this fuzz turned up (CHANGELOG, profiles/families_fuzz_soak.txt); the first five also run inside
    their blocks. 0 (gatv2, C = 192, xr one float into a flat buffer), 25 (transformer, C = 256, q and k one and three
    floats in), 338 (supergat, C = 132, h two floats in): an operand off the grid of the vector width a head of more than
    64 channels needs; the entry points refused the head ("needs N lanes per head") although *_supported takes it, until
    ops._rows_on_grid copied such operands. 51 (faconv, C = 256, x three floats in): refused by faconv.hip's alignment
    check, same cure. 15 (weighted, ops.propagate_gcn_edge_weight with two self-loops on one node): the kernels give the
    overwritten loop's weight a gradient of 0, which is right; the oracle's indexed assignment gave it one, and the
    reference was mended. 2291 (faconv, composed form, two nodes, 3070 copies of one edge): fa_edge_dot_kernel added a
    whole row into one accumulator and g_att_r came out 2.6e-4 of its scale off; it now sums runs of 64 slots.
    4168 (gatv2, two nodes, 1024 copies of one edge in a hub row): g_att 4.2e-4 off through the drift of the row's
    aggregate, which duplicate_rows now keeps out of the gradients. 1804 (gru, form='composed', x a column block of a
    wider matrix, 33 nodes): the strided state reaches the composed step's kernels as a view since ops._rows_on_grid
    replaced the step's .contiguous()."""
    run_family_case(dev, seed)
