"""ResGatedGraphConv on the host: a float64 restatement of the layer (per-channel gate sigmoid(k_i + q_j) on the value
row, summed over the in-edges AS GIVEN, root skip, bias) pinned by numbers derived by hand; registry, module layout
(PyG's names, strict state_dict loading), refusals and the C ABI of the new entry points; and the case builders
tests/test_gpu_resgated.py feeds to the HIP kernels, with the checks that keep those cases well-posed. No GPU needed.

Well-posedness. Every operator, saturated, layer and model case is run through the restatement in float32 on the CPU,
with the edges in REVERSED order (another summation order), and has to stay within a QUARTER of the GPU test's
tolerances (forward 1e-4, gradients 2e-4, times max(1, |ref|max)) of the float64 result: a condition on the inputs, not
on a kernel.

Input scales. k, q, v and the cotangent of the operator cases are N(0, 1) times OPERATOR_SCALE = 1 (a power of two): the
gate's argument k_i + q_j has standard deviation 1.4, so the gates sit on the sigmoid's slope, and the hub rows of
`powerlaw` (up to 1755 terms of order 1, nothing normalises them) use at most 0.03 of the tolerance in float32
(printed by test_operator_case_is_well_posed; the sums grow like sqrt(degree) and so does max |ref|, which the
tolerance scales with). The saturated case multiplies k and q by SATURATED_SCALE = 128: |k_i + q_j| runs into the
hundreds, beyond 88.7 = log FLT_MAX, where a sigmoid written 1 / (1 + exp(-z)) meets an infinite intermediate."""
import copy
import functools
import itertools
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from rgb_experiment_amd.models import ResGatedGCN       # without the feature this file fails here, at import
from rgb_experiment_amd.nn import ResGatedGraphConv

import test_transformer_host as T
from test_transformer_host import (FWD_TOL, GRAD_TOL, WELL_POSED_SHARE, f32_exact, graph_of, share_of_tolerance,
                                   slots_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------

def aggregate(k, q, v, n, src, dst):
    """out [n, C] = sum over the edges (src -> dst) as given of sigmoid(k[dst] + q[src]) * v[src], in the precision of
    the inputs; a node without in-edges gets zeros. The sum runs in the order of the edge list."""
    msg = torch.sigmoid(k.index_select(0, dst) + q.index_select(0, src)) * v.index_select(0, src)
    return torch.zeros(n, k.size(1), dtype=k.dtype).index_add(0, dst, msg)


class RefResGatedGraphConv(nn.Module):
    """float64 restatement of ResGatedGraphConv, written from the formulas of the layer's contract; PyG's parameter
    names (the three projections carry a bias, lin_skip has none and exists only with root_weight, `bias` only with
    bias)."""

    def __init__(self, in_channels, out_channels, root_weight=True, bias=True):
        super().__init__()
        self.lin_key = nn.Linear(in_channels, out_channels).double()
        self.lin_query = nn.Linear(in_channels, out_channels).double()
        self.lin_value = nn.Linear(in_channels, out_channels).double()
        self.lin_skip = nn.Linear(in_channels, out_channels, bias=False).double() if root_weight else None
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels, dtype=torch.float64))
        else:
            self.register_parameter("bias", None)

    def forward(self, x, ei, reverse=False):
        src, dst = (ei[0].flip(0), ei[1].flip(0)) if reverse else (ei[0], ei[1])
        out = aggregate(self.lin_key(x), self.lin_query(x), self.lin_value(x), x.size(0), src, dst)
        if self.lin_skip is not None:
            out = out + self.lin_skip(x)
        if self.bias is not None:
            out = out + self.bias
        return out


class RefResGatedGCN(nn.Module):
    """models/resgated.py in float64: (ResGatedGraphConv -> BatchNorm1d) x (L - 1), ResGatedGraphConv(hid, out); the
    product's module names."""

    def __init__(self, num_layers, hidden_unit, input_dim, output_dim, **kw):
        super().__init__()
        widths = [input_dim] + [hidden_unit] * (num_layers - 1) + [output_dim]
        self.convs = nn.ModuleList(RefResGatedGraphConv(widths[i], widths[i + 1], **kw) for i in range(num_layers))
        self.bns = nn.ModuleList(nn.BatchNorm1d(hidden_unit).double() for _ in range(num_layers - 1))

    def forward(self, x, ei, reverse=False):
        for i, conv in enumerate(self.convs):
            x = conv(x, ei, reverse)
            if i < len(self.bns):
                x = self.bns[i](x)
        return {"out": F.log_softmax(x, dim=1), "emb": x}


# ---- cases shared with tests/test_gpu_resgated.py -------------------------------------------------------------------

WIDTHS = [1, 4, 7, 5, 40, 64, 66, 128, 132, 256]   # every vector width (1, 2, 4) and 64, 8, 4, 2, 1 rows per wave-instruction
GRAPH_NAMES = T.GRAPH_NAMES                        # no_edges, powerlaw, random (tests/test_transformer_host.graph_of)
OPERATOR_SCALE = 1.0
SATURATED_WIDTHS = [8, 64]
SATURATED_GRAPHS = ("random", "powerlaw")
SATURATED_SCALE = 128.0
NAMES = ("forward", "g_k", "g_q", "g_v")


@functools.lru_cache(maxsize=None)
def operator_case(C, graph_name, saturated=False):
    """k, q, v [n, C] and the cotangent: float64, fp32-exact. `saturated`: k and q times SATURATED_SCALE."""
    _, n = graph_of(graph_name)
    g = torch.Generator().manual_seed(4000 + C)
    k, q, v, cot = (f32_exact((n, C), g, OPERATOR_SCALE) for _ in range(4))
    return (k * SATURATED_SCALE, q * SATURATED_SCALE, v, cot) if saturated else (k, q, v, cot)


def run_formula(case, graph_name, dtype=torch.float64, reverse=False):
    """The restatement's aggregation on a case in `dtype`: (out [n, C], [g_k, g_q, g_v]). `reverse`: the edge list
    backwards, i.e. every row summed in the opposite order."""
    _, n = graph_of(graph_name)
    src, dst, _, _ = slots_of(graph_name)
    if reverse:
        src, dst = src.flip(0), dst.flip(0)
    k, q, v = (t.to(dtype).clone().requires_grad_(True) for t in case[:3])
    out = aggregate(k, q, v, n, src, dst)
    (out * case[3].to(dtype)).sum().backward()
    return out.detach(), [k.grad, q.grad, v.grad]


@functools.lru_cache(maxsize=None)
def reference(C, graph_name, saturated=False):
    """The float64 result of a case, computed once and shared (read-only) by the host and the GPU tests."""
    return run_formula(operator_case(C, graph_name, saturated), graph_name)


def shares_of(got, want):
    out = {"forward": share_of_tolerance(got[0], want[0], FWD_TOL)}
    for name, a, b in zip(NAMES[1:], got[1], want[1]):
        out[name] = share_of_tolerance(a, b, GRAD_TOL)
    return out


LAYER_N, LAYER_E, LAYER_F = 120, 500, 10
LAYER_WIDTHS = [7, 67, 130]                       # 67 and 130 are outside the kernels' widths: the layer pads them
LAYER_FLAGS = list(itertools.product([True, False], repeat=2))   # root_weight x bias


def layer_case(C, root_weight, bias):
    """(x float64 fp32-exact, edge_index, reference layer with every parameter set to fp32-exact random values)."""
    from test_gpu_ggnn import rand_graph
    g = torch.Generator().manual_seed(8100 + C)
    ei = rand_graph(LAYER_N, LAYER_E, 8100, loops=5, dups=12)
    x = f32_exact((LAYER_N, LAYER_F), g)
    ref = RefResGatedGraphConv(LAYER_F, C, root_weight=root_weight, bias=bias)
    with torch.no_grad():
        for key, prm in ref.named_parameters():
            prm.copy_(f32_exact(prm.shape, g, prm.size(-1) ** -0.5 if key.endswith("weight") else 0.5))
    return x, ei, ref


MODEL_SHAPE = dict(n=60, e=240, f=16, hidden=12, classes=5, layers=3)


def model_case(**kw):
    """(x, y, edge_index of `random`-like shape, the product's model on the CPU, the reference holding its parameters)."""
    from test_gpu_ggnn import rand_graph
    s = MODEL_SHAPE
    g = torch.Generator().manual_seed(9200)
    ei = rand_graph(s["n"], s["e"], 9200, loops=3, dups=6)
    x = f32_exact((s["n"], s["f"]), g)
    y = torch.randint(0, s["classes"], (s["n"],), generator=g)
    torch.manual_seed(9200)
    model = ResGatedGCN(s["layers"], s["hidden"], s["f"], s["classes"], 0.0, **kw)
    with torch.no_grad():  # biases off zero, so that their paths are exercised
        for key, prm in model.named_parameters():
            if key.endswith("bias"):
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.3)
    ref = RefResGatedGCN(s["layers"], s["hidden"], s["f"], s["classes"], **kw)
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()},
                        strict=True)
    return x, y, ei, model, ref


# ---- the restatement is pinned -------------------------------------------------------------------------------------

L3 = 1.0986122886681098  # log 3: sigmoid(L3) = 3/4, sigmoid(-L3) = 1/4, sigmoid(0) = 1/2


def hand_inputs():
    t = lambda rows: torch.tensor(rows, dtype=torch.float64)
    k = t([[0, 0], [L3, 0], [0, -L3], [5, 5]])
    q = t([[0, L3], [-L3, 0], [7, 7], [9, 9]])
    v = t([[4, -8], [8, 4], [100, 100], [1000, 1000]])
    return k, q, v


def test_restatement_on_a_path():
    """0 -> 1 -> 2, two channels. Derived with scalar arithmetic from the contract's formula:
      out_1 = sigmoid(k_1 + q_0) * v_0 = sigmoid((L3, 0) + (0, L3)) * (4, -8) = (3/4, 3/4) * (4, -8) = (3, -6)
      out_2 = sigmoid(k_2 + q_1) * v_1 = sigmoid((0, -L3) + (-L3, 0)) * (8, 4) = (1/4, 1/4) * (8, 4) = (2, 1)
      out_0 = 0 (no in-edge).
    d out_2 / d k_2 = s (1 - s) v_1 = 3/16 * (8, 4) = (1.5, 0.75); k_0 reaches no output."""
    k, q, v = hand_inputs()
    k = k[:3].clone().requires_grad_(True)
    out = aggregate(k, q[:3], v[:3], 3, torch.tensor([0, 1]), torch.tensor([1, 2]))
    want = torch.tensor([[0, 0], [3, -6], [2, 1]], dtype=torch.float64)
    assert torch.allclose(out, want, rtol=0, atol=1e-12) and out[0].abs().max().item() == 0.0
    out[2].sum().backward()
    assert torch.allclose(k.grad, torch.tensor([[0, 0], [0, 0], [1.5, 0.75]], dtype=torch.float64), rtol=0, atol=1e-12)


def test_restatement_duplicate_self_loop_isolated():
    """Edges 0 -> 1 twice (a duplicate), 1 -> 1 (a self-loop), 1 -> 2; node 0 has no in-edge, node 3 no edge at all.
      out_1 = 2 * sigmoid(k_1 + q_0) * v_0 + sigmoid(k_1 + q_1) * v_1
            = 2 * (3, -6) + sigmoid((L3, 0) + (-L3, 0)) * (8, 4) = (6, -12) + (1/2, 1/2) * (8, 4) = (10, -10)
      out_2 = (2, 1) as on the path; out_0 = out_3 = 0.
    Through the layer, the isolated node's output is lin_skip(x_3) + bias and nothing else."""
    k, q, v = hand_inputs()
    src, dst = torch.tensor([0, 1, 0, 1]), torch.tensor([1, 1, 1, 2])
    out = aggregate(k, q, v, 4, src, dst)
    want = torch.tensor([[0, 0], [10, -10], [2, 1], [0, 0]], dtype=torch.float64)
    assert torch.allclose(out, want, rtol=0, atol=1e-12)
    assert out[0].abs().max().item() == 0.0 and out[3].abs().max().item() == 0.0
    once = aggregate(k, q, v, 4, src[1:], dst[1:])                       # the duplicate dropped: one share less
    assert torch.allclose(out[1] - once[1], torch.tensor([3.0, -6.0], dtype=torch.float64), rtol=0, atol=1e-12)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 3, generator=g, dtype=torch.float64)
    for root_weight, bias in LAYER_FLAGS:
        conv = RefResGatedGraphConv(3, 2, root_weight=root_weight, bias=bias)
        if bias:
            with torch.no_grad():
                conv.bias.copy_(torch.tensor([0.25, -0.5]))
        got = conv(x, torch.stack([src, dst]))
        alone = torch.zeros(2, dtype=torch.float64)
        if root_weight:
            alone = alone + x[3] @ conv.lin_skip.weight.t()
        if bias:
            alone = alone + conv.bias
        assert torch.allclose(got[3], alone, rtol=0, atol=1e-15)
        agg = aggregate(conv.lin_key(x), conv.lin_query(x), conv.lin_value(x), 4, src, dst)
        assert agg[1].abs().max().item() > 0 and not torch.allclose(got[1], alone)


def test_restatement_sums_in_either_order():
    case = operator_case(7, "random")
    a, b = run_formula(case, "random"), run_formula(case, "random", reverse=True)
    assert (a[0] - b[0]).abs().max().item() < 1e-12
    assert not torch.equal(run_formula(case, "random", torch.float32)[0],
                           run_formula(case, "random", torch.float32, reverse=True)[0])   # the order is another one


# ---- registry, module layout, refusals ---------------------------------------------------------------------------------

def test_registry():
    from rgb_experiment_amd.dist import experiment as dist_experiment
    from rgb_experiment_amd.initial_params import InitialParameters
    from rgb_experiment_amd.models import MODELS, REGISTRY
    from rgb_experiment_amd import nn as rnn
    assert MODELS["resgated"] is ResGatedGCN and "resgated" not in REGISTRY
    assert "resgated" not in dist_experiment.SUPPORTED
    assert len(InitialParameters.model_names) == 13
    assert "ResGatedGraphConv" in rnn.__all__


def pyg_shaped_state(f, C, root_weight, bias):
    """Names and shapes of PyG's ResGatedGraphConv.state_dict() for these keywords."""
    shapes = {}
    for name in ("lin_key", "lin_query", "lin_value"):
        shapes[name + ".weight"], shapes[name + ".bias"] = (C, f), (C,)
    if root_weight:
        shapes["lin_skip.weight"] = (C, f)
    if bias:
        shapes["bias"] = (C,)
    return shapes


@pytest.mark.parametrize("root_weight,bias", LAYER_FLAGS)
def test_state_dict_layout_and_strict_loading(root_weight, bias):
    kw = dict(root_weight=root_weight, bias=bias)
    conv = ResGatedGraphConv(6, 5, **kw)
    shapes = pyg_shaped_state(6, 5, **kw)
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == shapes
    assert (conv.lin_skip is not None) == root_weight and (conv.bias is not None) == bias
    if bias:
        assert conv.bias.abs().max().item() == 0.0                         # initialised with zeros
    assert conv.lin_key.bias.abs().max().item() > 0.0                      # the Linear's own initialisation
    g = torch.Generator().manual_seed(1)
    state = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    conv.load_state_dict(state, strict=True)
    ref = RefResGatedGraphConv(6, 5, **kw)
    ref.load_state_dict({k: v.double() for k, v in conv.state_dict().items()}, strict=True)
    conv.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    assert sorted(dict(conv.named_parameters())) == sorted(dict(ref.named_parameters()))
    assert all(torch.equal(conv.state_dict()[k], state[k]) for k in state)


def test_model_layout():
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    for kw in (dict(), dict(root_weight=False), dict(bias=False)):
        model = ResGatedGCN(3, 4, 10, 5, 0.5, **kw)
        assert all(isinstance(c, ResGatedGraphConv) for c in model.convs) and len(model.convs) == 3
        assert len(model.bns) == 2 and model.dropout_rate == 0.5
        assert shapes(model)["convs.0.lin_key.weight"] == (4, 10) and shapes(model)["convs.2.lin_value.weight"] == (5, 4)
        assert ("convs.1.lin_skip.weight" in shapes(model)) == kw.get("root_weight", True)
        assert ("convs.1.bias" in shapes(model)) == kw.get("bias", True)
        ref = RefResGatedGCN(3, 4, 10, 5, **kw)
        ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()},
                            strict=True)
        model.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()},
                              strict=True)
    x, y, ei, model, ref = model_case()
    res = ref(x, ei)
    assert set(res) == {"out", "emb"} and res["out"].shape == (MODEL_SHAPE["n"], MODEL_SHAPE["classes"])


def test_refusals():
    import rgb_experiment_amd as R
    from rgb_experiment_amd import ops
    with pytest.raises(NotImplementedError, match="edge_dim"):
        ResGatedGraphConv(4, 4, edge_dim=3)
    for act in (torch.tanh, torch.relu, nn.ReLU(), "sigmoid"):
        with pytest.raises(NotImplementedError, match="act"):
            ResGatedGraphConv(4, 4, act=act)
    for act in (None, torch.sigmoid, nn.Sigmoid()):                       # the default, spelled out
        ResGatedGraphConv(4, 4, act=act)
    conv = ResGatedGraphConv(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(torch.randn(5, 4), torch.tensor([[0, 1], [1, 2]]))

    class Partitioned:
        is_distributed = True
    t = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="no node-partitioned form"):
        ops.resgated_aggregate(t, t, t, Partitioned())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resgated_aggregate(t, t, t, object())
    g = torch.Generator().manual_seed(0)
    data = R.Data(x=torch.randn(30, 6, generator=g), y=torch.randint(0, 3, (30,), generator=g),
                  edge_index=torch.randint(0, 30, (2, 90), generator=g))
    params = {"num_layers": 2, "hidden_unit": 4, "dropout_rate": 0.0}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.experiment(params, specify_data=True, data=data, model_name="resgated", use_cpu=True, print_print=False)
    with pytest.raises(NotImplementedError, match="no node-partitioned form"):
        R.experiment(params, specify_data=True, data=data, model_name="resgated", distributed=True, print_print=False)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

NEW_ENTRIES = ("rgbx_resgated_supported", "rgbx_resgated_fwd_f32", "rgbx_resgated_bwd_dst_f32",
               "rgbx_resgated_bwd_src_f32")


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
        assert bool(lib.rgbx_resgated_supported(C)) == bool(lib.rgbx_transformer_supported(1, C)), C
    assert not lib.rgbx_resgated_supported(0) and not lib.rgbx_resgated_supported(-4)
    assert all(lib.rgbx_resgated_supported(C) for C in WIDTHS)
    assert not any(lib.rgbx_resgated_supported(C) for C in (67, 130, 260))
    p = 0x10000  # 16-byte aligned, non-null, never dereferenced: every call below returns before a launch

    def fwd(**kw):
        a = dict(rowptr=p, col=p, k=p, ldk=64, q=p, ldq=64, v=p, ldv=64, out=p, ldo=64, N=10, C=64)
        a.update(kw)
        return lib.rgbx_resgated_fwd_f32(a["rowptr"], a["col"], a["k"], a["ldk"], a["q"], a["ldq"], a["v"], a["ldv"],
                                         a["out"], a["ldo"], a["N"], a["C"], None, None)
    assert fwd(rowptr=None) == -1 and b"null" in lib.rgbx_last_error_string()
    assert fwd(col=None) == -1 and fwd(k=None) == -1 and fwd(q=None) == -1 and fwd(v=None) == -1
    assert fwd(out=None) == -1
    assert fwd(ldk=63) == -1 and b"leading dimension" in lib.rgbx_last_error_string()
    assert fwd(ldq=32) == -1 and fwd(ldv=63) == -1 and fwd(ldo=8) == -1
    assert fwd(N=-1) == -1 and fwd(C=0) == -1
    assert fwd(N=2 ** 31) == -2                                           # RGBX_E_RANGE
    assert fwd(C=67, ldk=67, ldq=67, ldv=67, ldo=67) == -5                # RGBX_E_SHAPE
    assert fwd(C=130, ldk=130, ldq=130, ldv=130, ldo=130) == -5 and fwd(C=1000) == -5
    assert fwd(v=p + 2) == -3 and b"aligned" in lib.rgbx_last_error_string()   # RGBX_E_ALIGN
    assert fwd(k=p + 1) == -3 and fwd(out=p + 3) == -3
    # C = 256 needs 4 floats per lane: 16-byte pointers and leading dimensions that are multiples of 4
    wide = dict(C=256, ldk=256, ldq=256, ldv=256, ldo=256)
    assert fwd(**{**wide, "q": p + 8}) == -5 and b"lanes" in lib.rgbx_last_error_string()
    assert fwd(**{**wide, "ldv": 258}) == -5
    assert fwd(N=0) == 0 and fwd(N=0, rowptr=None) == 0                   # nothing to do

    def dst(**kw):
        a = dict(k=p, q=p, v=p, gout=p, ldg=64, g_k=p, ldgk=64, N=1000, C=64)
        a.update(kw)
        return lib.rgbx_resgated_bwd_dst_f32(p, p, a["k"], 64, a["q"], 64, a["v"], 64, a["gout"], a["ldg"], a["g_k"],
                                             a["ldgk"], a["N"], a["C"], None, None)
    assert dst(k=None) == -1 and dst(q=None) == -1 and dst(v=None) == -1 and dst(gout=None) == -1
    assert dst(g_k=None) == -1
    assert dst(ldg=32) == -1 and dst(ldgk=63) == -1
    assert dst(gout=p + 2) == -3 and dst(g_k=p + 1) == -3
    assert dst(C=67) == -5
    assert dst(N=2 ** 31) == -2 and dst(N=0) == 0

    def src(**kw):
        a = dict(k=p, q=p, v=p, gout=p, g_q=p, ldgq=64, g_v=p, ldgv=64, N=1000, C=64)
        a.update(kw)
        return lib.rgbx_resgated_bwd_src_f32(p, p, a["k"], 64, a["q"], 64, a["v"], 64, a["gout"], 64, a["g_q"],
                                             a["ldgq"], a["g_v"], a["ldgv"], a["N"], a["C"], None, None)
    assert src(k=None) == -1 and src(q=None) == -1 and src(v=None) == -1 and src(gout=None) == -1
    assert src(g_q=None) == -1 and src(g_v=None) == -1
    assert src(ldgq=63) == -1 and src(ldgv=32) == -1
    assert src(g_v=p + 2) == -3 and src(g_q=p + 1) == -3
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


@pytest.mark.parametrize("graph", GRAPH_NAMES)
@pytest.mark.parametrize("C", WIDTHS)
def test_operator_case_is_well_posed(C, graph):
    want = reference(C, graph)
    low = run_formula(operator_case(C, graph), graph, torch.float32, reverse=True)
    shares = shares_of(low, want)
    print(f"C = {C} {graph}: max |out| {want[0].abs().max().item():.1f}; float32 (reversed order) vs float64 share of "
          f"tolerance {shares}")
    assert all(torch.isfinite(t).all() for t in [low[0]] + low[1])
    assert max(shares.values()) <= WELL_POSED_SHARE, shares
    ei, n = graph_of(graph)
    if graph == "no_edges":
        assert all(t.abs().max().item() == 0.0 for t in [want[0]] + want[1])
    if graph == "random":      # rows without in-edges, sources without out-edges: exact zeros in the reference too
        assert want[0][:20].abs().max().item() == 0.0 and want[1][0][:20].abs().max().item() == 0.0
        assert want[1][1][20:40].abs().max().item() == 0.0 and want[1][2][20:40].abs().max().item() == 0.0
    if graph == "powerlaw":    # the hub rows are not convex combinations: they grow with the degree
        hub = int(torch.bincount(ei[1], minlength=n).argmax())
        assert want[0][hub].abs().max().item() > 10.0


@pytest.mark.parametrize("graph", SATURATED_GRAPHS)
@pytest.mark.parametrize("C", SATURATED_WIDTHS)
def test_saturated_case_is_saturated_and_well_posed(C, graph):
    """k, q of standard deviation 128: at least half of the float32 gates are exactly 0 or 1, arguments beyond the range
    of an unguarded expf occur in numbers, the float64 gradients are finite and float32 stays inside a quarter of the
    unchanged tolerance."""
    case = operator_case(C, graph, saturated=True)
    assert abs(case[0].std().item() - SATURATED_SCALE) < 0.05 * SATURATED_SCALE
    assert abs(case[1].std().item() - SATURATED_SCALE) < 0.05 * SATURATED_SCALE
    src, dst, _, _ = slots_of(graph)
    z = case[0].float()[dst] + case[1].float()[src]
    s = torch.sigmoid(z)
    exact = ((s == 0.0) | (s == 1.0)).float().mean().item()
    beyond = int((z.abs() > 88.8).sum())
    want = reference(C, graph, saturated=True)
    low = run_formula(case, graph, torch.float32, reverse=True)
    shares = shares_of(low, want)
    print(f"saturated C = {C} {graph}: max |z| {z.abs().max().item():.0f}, {beyond} of {z.numel()} beyond log FLT_MAX, "
          f"share of gates exactly 0 or 1 {exact:.3f}; float32 vs float64 share of tolerance {shares}")
    assert exact >= 0.5 and z.abs().max().item() > 300 and beyond >= 1000
    assert not bool(torch.isfinite(torch.exp(-z)).all())                   # 1 / (1 + exp(-z)) meets an inf in float32
    assert all(torch.isfinite(t).all() for t in [want[0]] + want[1])
    assert all(torch.isfinite(t).all() for t in [low[0]] + low[1])
    assert max(shares.values()) <= WELL_POSED_SHARE, shares


@pytest.mark.parametrize("root_weight,bias", LAYER_FLAGS)
@pytest.mark.parametrize("C", LAYER_WIDTHS)
def test_layer_case_is_well_posed(C, root_weight, bias):
    x, ei, ref = layer_case(C, root_weight, bias)
    cot = f32_exact((LAYER_N, C), torch.Generator().manual_seed(17))
    low = copy.deepcopy(ref).float()
    x64, x32 = x.clone().requires_grad_(True), x.float().requires_grad_(True)
    want, got = ref(x64, ei), low(x32, ei, reverse=True)
    (want * cot).sum().backward()
    (got * cot.float()).sum().backward()
    shares = {"forward": share_of_tolerance(got, want, FWD_TOL), "x": share_of_tolerance(x32.grad, x64.grad, GRAD_TOL)}
    lowp = dict(low.named_parameters())
    for key, prm in ref.named_parameters():
        shares[key] = share_of_tolerance(lowp[key].grad, prm.grad, GRAD_TOL)
    print(f"C = {C} root_weight={root_weight} bias={bias}: {shares}")
    assert len(shares) == 2 + 6 + root_weight + bias
    assert max(shares.values()) <= WELL_POSED_SHARE, shares
    assert int((torch.bincount(ei[1], minlength=LAYER_N) == 0).sum()) > 0   # nodes without in-edges


def test_model_case_is_well_posed():
    x, y, ei, model, ref = model_case()
    ref.train()
    low = copy.deepcopy(ref).float()
    want, got = ref(x, ei), low(x.float(), ei, reverse=True)
    F.nll_loss(want["out"], y).backward()
    F.nll_loss(got["out"], y).backward()
    shares = {"emb": share_of_tolerance(got["emb"], want["emb"], FWD_TOL),
              "out": share_of_tolerance(got["out"], want["out"], FWD_TOL)}
    lowp = dict(low.named_parameters())
    for key, prm in ref.named_parameters():
        shares[key] = share_of_tolerance(lowp[key].grad, prm.grad, GRAD_TOL)
    print(shares)
    assert max(shares.values()) <= WELL_POSED_SHARE, shares
