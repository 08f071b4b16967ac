"""GATv2 on the host: a float64 restatement of GATv2Conv (dynamic attention) pinned by numbers computed by hand and, in
the degenerate case where the score factors, by the oracle's GATConv; registry, module layout (PyG's names, strict
state_dict loading), refusals and the C ABI of the new entry points. No GPU needed."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rewritten_edges(ei, n):
    """Self-loops removed, one self-loop per node appended (add_self_loops=True): (src, dst)."""
    keep = ei[0] != ei[1]
    loops = torch.arange(n, dtype=ei.dtype)
    return torch.cat([ei[0][keep], loops]), torch.cat([ei[1][keep], loops])


class RefGATv2Conv(nn.Module):
    """float64 restatement of GATv2Conv with add_self_loops=True, written from the formulas of the layer's contract;
    PyG's parameter names. The dropout decisions are INPUTS (`choices`): 'src' / 'dst' (the edges after the self-loop
    rewrite, in the order the mask refers to) and 'keep' bool [E', H] (True = kept). Without `choices` the edges are
    rewritten here and nothing is dropped. `self.s` keeps the pre-activations [E', H, C] of the last forward."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, bias=True,
                 share_weights=False):
        super().__init__()
        self.H, self.C, self.concat, self.slope, self.p = heads, out_channels, concat, negative_slope, dropout
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=bias).double()
        self.lin_r = self.lin_l if share_weights else nn.Linear(in_channels, heads * out_channels, bias=bias).double()
        self.att = nn.Parameter(torch.randn(1, heads, out_channels, dtype=torch.float64))
        if bias:
            self.bias = nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels, dtype=torch.float64))
        else:
            self.register_parameter("bias", None)

    def attend(self, xl, xr, n, src, dst, keep=None):
        """out [n, H, C] from x_l, x_r [n, H, C] (no bias, heads not merged)."""
        H = self.H
        s = xl[src] + xr[dst]                                                        # [E', H, C]
        e = (self.att * F.leaky_relu(s, self.slope)).sum(-1)                         # [E', H]
        idx = dst.view(-1, 1).expand(-1, H)
        mx = torch.full((n, H), -1e30, dtype=torch.float64).scatter_reduce(0, idx, e.detach(), "amax")
        ex = torch.exp(e - mx[dst])
        den = torch.zeros(n, H, dtype=torch.float64).index_add(0, dst, ex)
        alpha = ex / (den[dst] + 1e-16)
        self.s, self.e, self.alpha = s.detach(), e.detach(), alpha.detach()
        if keep is not None:
            alpha = alpha * keep.double() / (1.0 - self.p)
        return torch.zeros(n, H, self.C, dtype=torch.float64).index_add(0, dst, alpha.unsqueeze(-1) * xl[src])

    def forward(self, x, ei, choices=None):
        n, H, C = x.size(0), self.H, self.C
        src, dst = rewritten_edges(ei, n) if choices is None else (choices["src"], choices["dst"])
        keep = choices["keep"] if (choices is not None and self.training and self.p > 0) else None
        out = self.attend(self.lin_l(x).view(n, H, C), self.lin_r(x).view(n, H, C), n, src, dst, keep)
        out = out.reshape(n, H * C) if self.concat else out.mean(1)
        return out if self.bias is None else out + self.bias


class RefGATv2(nn.Module):
    """models/gatv2.py in float64: (GATv2Conv -> BatchNorm1d) x (L - 1), GATv2Conv(hid * heads, out, 1, concat=False);
    the product's module names. `choices`: one entry per layer (None = nothing dropped)."""

    def __init__(self, num_layers, hidden_unit, input_dim, output_dim, heads, share_weights=False, att_dropout=0.0):
        super().__init__()
        wide = hidden_unit * heads
        kw = dict(dropout=att_dropout, share_weights=share_weights)
        self.convs = nn.ModuleList(
            [RefGATv2Conv(input_dim if i == 0 else wide, hidden_unit, heads, **kw) for i in range(num_layers - 1)]
            + [RefGATv2Conv(wide, output_dim, 1, concat=False, **kw)])
        self.bns = nn.ModuleList(nn.BatchNorm1d(wide).double() for _ in range(num_layers - 1))

    def forward(self, x, ei, choices=None):
        choices = [None] * len(self.convs) if choices is None else choices
        for i, conv in enumerate(self.convs):
            x = conv(x, ei, choices[i])
            if i < len(self.bns):
                x = self.bns[i](x)
        return {"out": F.log_softmax(x, dim=1), "emb": x}

    def near_kink(self, bound=1e-4):
        """How many (slot, head, channel) pre-activations of the last forward lie within `bound` of LeakyReLU's kink."""
        return [int((conv.s.abs() < bound).sum()) for conv in self.convs]


def test_restatement_reproduces_hand_computed_numbers():
    """3 nodes, 3 edges, one head of two channels, W_l = I, W_r = diag(0.5, -1), att = (1, -0.5), slope 0.2. Every
    number below was computed edge by edge with scalar arithmetic from the contract's formulas (s, leaky_relu, e,
    softmax per target, weighted sum), not with the class under test."""
    x = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], dtype=torch.float64)
    ei = torch.tensor([[0, 2, 1], [1, 1, 2]])
    conv = RefGATv2Conv(2, 2, heads=1, bias=False)
    with torch.no_grad():
        conv.lin_l.weight.copy_(torch.eye(2))
        conv.lin_r.weight.copy_(torch.tensor([[0.5, 0.0], [0.0, -1.0]]))
        conv.att.copy_(torch.tensor([[[1.0, -0.5]]]))
    conv.eval()
    out = conv(x, ei)
    # slots after the rewrite: 0->1, 2->1, 1->2, then the self-loops 0, 1, 2
    # x_r = (0.5, 0), (0, -1), (0.5, -1)
    want_s = [[1.0, -1.0], [1.0, 0.0], [0.5, 0.0], [1.5, 0.0], [0.0, 0.0], [1.5, 0.0]]
    want_e = [1.1, 1.0, 0.5, 1.5, 0.0, 1.5]
    # target 1: exp(1.1), exp(1.0), exp(0) -> / 6.722448; target 2: exp(0.5), exp(1.5) -> / 6.130410
    want_alpha = [0.446886, 0.404356, 0.268941, 1.0, 0.148755, 0.731059]
    want_out = [[1.0, 0.0], [0.851242, 0.553111], [0.731059, 1.0]]
    t = lambda v: torch.tensor(v, dtype=torch.float64)
    assert torch.allclose(conv.s[:, 0], t(want_s), atol=1e-12)
    assert torch.allclose(conv.e[:, 0], t(want_e), atol=1e-12)
    assert torch.allclose(conv.alpha[:, 0], t(want_alpha), atol=1e-6)
    assert torch.allclose(out, t(want_out), atol=1e-6)
    # dropout at p = 0.5 with slot 1 (2 -> 1) dropped: target 1 keeps 2 * (alpha_0 x_0 + alpha_4 x_1)
    conv.train()
    conv.p = 0.5
    src, dst = rewritten_edges(ei, 3)
    keep = torch.tensor([[1], [0], [1], [1], [1], [1]], dtype=torch.bool)
    out_d = conv(x, ei, {"src": src, "dst": dst, "keep": keep})
    assert torch.allclose(out_d[1], t([2 * 0.446886, 2 * 0.148755]), atol=1e-5)
    assert torch.allclose(out_d[0], t([2.0, 0.0]), atol=1e-12)


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("concat", [True, False])
def test_restatement_equals_the_oracle_gat_where_the_score_factors(heads, concat):
    """negative_slope = 1, shared weights, zero projection bias: e = <att, h_j + h_i> = <h_j, att> + <h_i, att>, which is
    GATConv with att_src = att_dst = att and the identity for LeakyReLU. oracle.ref_cpu.gat_conv is pinned to the
    goldens."""
    from oracle import ref_cpu
    n, f, c = 40, 6, 5
    g = torch.Generator().manual_seed(11 + heads)
    ei = torch.randint(0, n, (2, 200), generator=g)
    k = torch.randint(0, n, (7,), generator=g)
    ei = torch.cat([ei, torch.stack([k, k]), ei[:, :15]], dim=1)  # loops and duplicates
    x = torch.randn(n, f, generator=g, dtype=torch.float64)
    conv = RefGATv2Conv(f, c, heads=heads, concat=concat, negative_slope=1.0, share_weights=True).eval()
    with torch.no_grad():
        conv.lin_l.bias.zero_()
        conv.bias.copy_(torch.randn(conv.bias.shape, generator=g, dtype=torch.float64))
    got = conv(x, ei)
    want = ref_cpu.gat_conv(x, ei, conv.lin_l.weight.detach(), conv.att.detach(), conv.att.detach(), conv.bias.detach(),
                            heads, concat, negative_slope=1.0)
    assert (got - want).abs().max().item() < 1e-12


def test_state_dict_layout_and_strict_loading():
    from rgb_experiment_amd.models import GATv2
    from rgb_experiment_amd.nn import GATv2Conv
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}
    conv = GATv2Conv(6, 4, heads=3)
    assert shapes(conv) == {"att": (1, 3, 4), "bias": (12,), "lin_l.weight": (12, 6), "lin_l.bias": (12,),
                            "lin_r.weight": (12, 6), "lin_r.bias": (12,)}
    assert conv.lin_r is not conv.lin_l
    shared = GATv2Conv(6, 4, heads=3, share_weights=True)
    assert shared.lin_r is shared.lin_l
    assert {k: v for k, v in shapes(shared).items() if not k.startswith("lin_r")} == {
        "att": (1, 3, 4), "bias": (12,), "lin_l.weight": (12, 6), "lin_l.bias": (12,)}
    assert len(list(shared.parameters())) == 4  # the shared projection counts once
    nobias = GATv2Conv(6, 4, heads=3, bias=False)
    assert shapes(nobias) == {"att": (1, 3, 4), "lin_l.weight": (12, 6), "lin_r.weight": (12, 6)}
    assert nobias.bias is None and nobias.lin_l.bias is None
    mean = GATv2Conv(6, 4, heads=3, concat=False)
    assert shapes(mean)["bias"] == (4,) and shapes(mean)["lin_l.weight"] == (12, 6)
    # initialisation: glorot weights and att (inside their bounds), zero biases
    assert conv.bias.abs().max().item() == 0.0 and conv.lin_l.bias.abs().max().item() == 0.0
    assert conv.lin_r.bias.abs().max().item() == 0.0
    assert 0.0 < conv.att.abs().max().item() <= (6.0 / 7) ** 0.5
    assert 0.0 < conv.lin_l.weight.abs().max().item() <= (6.0 / 18) ** 0.5
    for kw in (dict(), dict(share_weights=True)):
        model = GATv2(3, 4, 10, 5, 0.5, 2, **kw)
        assert isinstance(model.convs[0], GATv2Conv) and model.convs[0].heads == 2 and model.convs[0].concat
        assert model.convs[-1].heads == 1 and not model.convs[-1].concat and len(model.bns) == 2
        assert shapes(model)["convs.1.lin_l.weight"] == (8, 8) and shapes(model)["convs.2.att"] == (1, 1, 5)
        ref = RefGATv2(3, 4, 10, 5, 2, **kw)
        ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()},
                            strict=True)
        model.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()},
                              strict=True)
    assert GATv2(2, 4, 10, 5, 0.5, 2, att_dropout=0.25).convs[1].dropout == 0.25


def test_refusals():
    import rgb_experiment_amd as R
    from rgb_experiment_amd.nn import GATv2Conv
    with pytest.raises(NotImplementedError, match="add_self_loops"):
        GATv2Conv(4, 4, add_self_loops=False)
    with pytest.raises(NotImplementedError, match="edge_dim"):
        GATv2Conv(4, 4, edge_dim=3)
    with pytest.raises(NotImplementedError, match="residual"):
        GATv2Conv(4, 4, residual=True)
    for p in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="dropout"):
            GATv2Conv(4, 4, dropout=p)
    conv = GATv2Conv(4, 3, heads=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(torch.randn(5, 4), torch.tensor([[0, 1], [1, 2]]))
    g = torch.Generator().manual_seed(0)
    data = R.Data(x=torch.randn(30, 6, generator=g), y=torch.randint(0, 3, (30,), generator=g),
                  edge_index=torch.randint(0, 30, (2, 90), generator=g))
    params = {"num_layers": 2, "hidden_unit": 4, "dropout_rate": 0.0, "heads": 2}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.experiment(params, specify_data=True, data=data, model_name="gatv2", use_cpu=True, print_print=False)


def test_registry():
    from rgb_experiment_amd.dist import experiment as dist_experiment
    from rgb_experiment_amd.initial_params import InitialParameters
    from rgb_experiment_amd.models import GATv2, MODELS, REGISTRY
    assert MODELS["gatv2"] is GATv2 and "gatv2" not in REGISTRY
    assert len(InitialParameters.model_names) == 13
    assert "gatv2" not in dist_experiment.SUPPORTED


NEW_ENTRIES = ("rgbx_gatv2_supported", "rgbx_gatv2_fwd_f32", "rgbx_gatv2_att_partial_floats", "rgbx_gatv2_bwd_dst_f32",
               "rgbx_gatv2_bwd_src_f32", "rgbx_gatv2_draws_u8")


def test_abi_declares_and_exports_the_new_entries():
    from rgb_experiment_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbx_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rgbx_[a-z0-9_]+)\s*\(", text))
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS, name
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.rgbx_version() == 501
    p = 0x10000  # 16-byte aligned, non-null, never dereferenced: every call below returns before a launch
    # widths: what GATConv.kernel_channels leaves unpadded
    ok = lib.rgbx_gatv2_supported
    assert ok(1, 4) and ok(1, 7) and ok(2, 8) and ok(8, 8) and ok(3, 5) and ok(8, 40) and ok(1, 64) and ok(1, 128)
    assert ok(1, 256) and ok(2, 66)
    assert not ok(1, 67) and not ok(2, 67) and not ok(1, 130) and not ok(1, 260) and not ok(0, 8) and not ok(8, 0)

    def fwd(**kw):
        a = dict(rowptr=p, xl=p, ldl=64, xr=p, att=p, out=p, m=p, rden=p, N=10, H=8, C=8, seed=None, p_drop=0.0)
        a.update(kw)
        return lib.rgbx_gatv2_fwd_f32(a["rowptr"], p, a["xl"], a["ldl"], a["xr"], 64, a["att"], None, a["out"], 64, a["m"],
                                      a["rden"], a["N"], a["H"], a["C"], 0.2, a["seed"], a["p_drop"], None, None)
    assert fwd(rowptr=None) == -1 and b"null" in lib.rgbx_last_error_string()
    assert fwd(xr=None) == -1 and fwd(att=None) == -1 and fwd(out=None) == -1
    assert fwd(ldl=32) == -1                               # leading dimension < H*C
    assert fwd(m=None) == -1                               # m without rden
    assert fwd(m=None, rden=None, seed=p) == -1            # the inference form has no dropout
    assert fwd(seed=p, p_drop=1.0) == -1
    assert fwd(N=-1) == -1 and fwd(H=0) == -1
    assert fwd(N=2 ** 31) == -2
    assert fwd(H=1, C=67, ldl=67) == -5 and fwd(H=1, C=1000, ldl=1000) == -5   # RGBX_E_SHAPE
    assert fwd(xl=p + 2) == -3 and b"aligned" in lib.rgbx_last_error_string()  # RGBX_E_ALIGN
    assert fwd(N=0) == 0                                   # nothing to do

    cnt = ctypes.c_int64(0)
    assert lib.rgbx_gatv2_att_partial_floats(1000, 8, 8, None, ctypes.byref(cnt)) == 0 and cnt.value == 250 * 64
    assert lib.rgbx_gatv2_att_partial_floats(10 ** 8, 1, 4, None, ctypes.byref(cnt)) == 0 and cnt.value == 8192 * 4
    assert lib.rgbx_gatv2_att_partial_floats(1000, 8, 8, None, None) == -1
    assert lib.rgbx_gatv2_att_partial_floats(-1, 8, 8, None, ctypes.byref(cnt)) == -1

    def dst(**kw):
        a = dict(xl=p, ldg=64, nodeq=p, g_xr=p, g_att=p, part=p, n_part=250 * 64, N=1000, C=8, seed=None, p_drop=0.0)
        a.update(kw)
        return lib.rgbx_gatv2_bwd_dst_f32(p, p, a["xl"], 64, p, 64, p, p, p, p, 64, None, p, a["ldg"], a["nodeq"],
                                          a["g_xr"], 64, a["g_att"], a["part"], a["n_part"], a["N"], 8, a["C"], 0.2,
                                          a["seed"], a["p_drop"], None, None)
    assert dst(xl=None) == -1 and dst(g_xr=None) == -1 and dst(g_att=None) == -1 and dst(part=None) == -1
    assert dst(ldg=32) == -1
    assert dst(nodeq=p + 4) == -3                          # the record is read as 8-byte pairs
    assert dst(xl=p + 1) == -3
    assert dst(n_part=250 * 64 - 1) == -4 and b"partial" in lib.rgbx_last_error_string()   # RGBX_E_WS
    assert dst(C=67) == -5
    assert dst(seed=p, p_drop=-0.5) == -1

    def src(**kw):
        a = dict(t2f=None, xr=p, ldgl=64, nodeq=p, g_xl=p, N=1000, C=8, seed=None, p_drop=0.0)
        a.update(kw)
        return lib.rgbx_gatv2_bwd_src_f32(p, p, a["t2f"], p, 64, a["xr"], 64, p, a["nodeq"], p, 64, a["g_xl"], a["ldgl"],
                                          a["N"], 8, a["C"], 0.2, a["seed"], a["p_drop"], None, None)
    assert src(xr=None) == -1 and src(g_xl=None) == -1 and src(nodeq=None) == -1
    assert src(ldgl=63) == -1
    assert src(seed=p, p_drop=0.5) == -1 and b"slot map" in lib.rgbx_last_error_string()
    assert src(nodeq=p + 4) == -3 and src(g_xl=p + 2) == -3
    assert src(C=130) == -5
    assert src(N=0) == 0

    assert lib.rgbx_gatv2_draws_u8(None, 5, 8, 0.5, p, None) == -1
    assert lib.rgbx_gatv2_draws_u8(p, 5, 0, 0.5, p, None) == -1
    assert lib.rgbx_gatv2_draws_u8(p, 2 ** 31, 8, 0.5, p, None) == -2
    assert lib.rgbx_gatv2_draws_u8(p, 0, 8, 0.5, p, None) == 0
