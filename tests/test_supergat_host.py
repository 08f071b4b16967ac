"""SuperGAT on the host: a float64 restatement of SuperGATConv ('MX' attention, attention loss) checked against numbers
computed by hand, registry, defaults, module layout (reference names, strict state_dict loading), refusals and the C
ABI of the new entry points. No GPU needed."""
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rewritten_edges(ei, n):
    """Self-loops removed, one self-loop per node appended (SuperGATConv's add_self_loops=True): (src, dst)."""
    keep = ei[0] != ei[1]
    loops = torch.arange(n, dtype=ei.dtype)
    return torch.cat([ei[0][keep], loops]), torch.cat([ei[1][keep], loops])


class RefSuperGATConv(nn.Module):
    """float64 restatement of SuperGATConv with attention_type='MX', add_self_loops=True, bias=True, written from the
    formulas of the layer's contract; same parameter names. Random choices are INPUTS (`choices`): 'src' / 'dst' (the
    edges after the self-loop rewrite, in the order the masks refer to), 'pos' bool [E'], 'drop' bool [E', H] (True =
    kept), 'neg' int64 [2, n], 'valid' bool [n]. Without `choices` in eval mode the edges are rewritten here."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0):
        super().__init__()
        self.H, self.C, self.concat, self.slope, self.p = heads, out_channels, concat, negative_slope, dropout
        self.lin = nn.Linear(in_channels, heads * out_channels, bias=False).double()
        self.att_l = nn.Parameter(torch.randn(1, heads, out_channels, dtype=torch.float64))
        self.att_r = nn.Parameter(torch.randn(1, heads, out_channels, dtype=torch.float64))
        self.bias = nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels, dtype=torch.float64))
        self.att_loss = None

    def forward(self, x, ei, choices=None):
        n, H, C = x.size(0), self.H, self.C
        if choices is None:
            assert not self.training, "a training forward needs its random choices"
            src, dst = rewritten_edges(ei, n)
        else:
            src, dst = choices["src"], choices["dst"]
        h = self.lin(x).view(n, H, C)
        hj, hi = h[src], h[dst]
        d = (hi * hj).sum(-1)                                                        # [E', H]
        s = ((hj * self.att_l).sum(-1) + (hi * self.att_r).sum(-1)) * torch.sigmoid(d)
        e = F.leaky_relu(s, self.slope)
        idx = dst.view(-1, 1).expand(-1, H)
        mx = torch.full((n, H), -1e30, dtype=torch.float64).scatter_reduce(0, idx, e.detach(), "amax")
        ex = torch.exp(e - mx[dst])
        den = torch.zeros(n, H, dtype=torch.float64).index_add(0, dst, ex)
        alpha = ex / (den[dst] + 1e-16)
        self.d, self.s, self.alpha = d, s, alpha
        if self.training:
            alpha = alpha * choices["drop"].double() / (1.0 - self.p)
        out = torch.zeros(n, H, C, dtype=torch.float64).index_add(0, dst, alpha.unsqueeze(-1) * hj)
        out = out.reshape(n, H * C) if self.concat else out.mean(1)
        if self.training:
            pos = d[choices["pos"]].mean(-1)
            u, v = choices["neg"][0][choices["valid"]], choices["neg"][1][choices["valid"]]
            neg = (h[u] * h[v]).sum(-1).mean(-1)
            logits = torch.cat([pos, neg])
            labels = torch.cat([torch.ones_like(pos), torch.zeros_like(neg)])
            self.att_loss = F.binary_cross_entropy_with_logits(logits, labels)
        else:
            self.att_loss = torch.zeros((), dtype=torch.float64)
        return out + self.bias


class RefSuperGAT(nn.Module):
    """reference models/supergat.py in float64. The feature dropouts are inputs too: `masks` = (mask0 [N, F], mask1
    [N, hidden * heads]) of 0 / 1 (None = no dropout), scaled by 1 / (1 - p) here."""

    def __init__(self, input_dim, hidden_dim, output_dim, heads, dropout_rate):
        super().__init__()
        self.p = dropout_rate
        self.conv1 = RefSuperGATConv(input_dim, hidden_dim, heads, True, dropout=dropout_rate)
        self.conv2 = RefSuperGATConv(hidden_dim * heads, output_dim, heads, False, dropout=dropout_rate)

    def forward(self, x, ei, choices=(None, None), masks=(None, None)):
        drop = lambda t, m: t if (m is None or not self.training) else t * m.double() / (1.0 - self.p)
        x = F.elu(self.conv1(drop(x, masks[0]), ei, choices[0]))
        x = self.conv2(drop(x, masks[1]), ei, choices[1])
        return {"out": F.log_softmax(x, dim=1), "emb": x, "att_loss": self.conv1.att_loss + self.conv2.att_loss}


def test_restatement_reproduces_hand_computed_numbers():
    """N = 5, one head of two channels, W = I. Every number below was computed edge by edge with scalar arithmetic from
    the contract's formulas (d, s, softmax per target, weighted sum, BCE), not with the class under test."""
    x = torch.tensor([[1.0, 0.5], [0.5, -1.0], [0.0, 2.0], [-1.0, 1.0], [0.25, 0.25]], dtype=torch.float64)
    ei = torch.tensor([[0, 4, 2, 1], [1, 4, 1, 3]])  # (4, 4): a self-loop of the input, removed and re-added
    conv = RefSuperGATConv(2, 2, heads=1)
    with torch.no_grad():
        conv.lin.weight.copy_(torch.eye(2))
        conv.att_l.copy_(torch.tensor([[[0.5, -0.25]]]))
        conv.att_r.copy_(torch.tensor([[[-0.5, 1.0]]]))
    conv.eval()
    out = conv(x, ei)
    # edges after the rewrite: 0->1, 2->1, 1->3, then the self-loops 0..4
    want_d = [0.0, -2.0, -1.5, 1.25, 1.25, 4.0, 2.0, 0.125]
    want_s = [-0.4375, -0.208605, 0.364851, 0.291487, -0.582975, 1.473021, 0.660598, 0.099602]
    want_alpha = [0.331327, 0.346847, 0.426598, 1.0, 0.321826, 1.0, 0.573402, 1.0]
    want_out = [[1.0, 0.5], [0.49224, 0.537532], [0.0, 2.0], [-0.360104, 0.146805], [0.25, 0.25]]
    assert torch.allclose(conv.d[:, 0], torch.tensor(want_d, dtype=torch.float64), atol=1e-6)
    assert torch.allclose(conv.s[:, 0], torch.tensor(want_s, dtype=torch.float64), atol=1e-6)
    assert torch.allclose(conv.alpha[:, 0], torch.tensor(want_alpha, dtype=torch.float64), atol=1e-6)
    assert torch.allclose(out, torch.tensor(want_out, dtype=torch.float64), atol=1e-6)
    assert conv.att_loss.item() == 0.0
    # training mode, nothing dropped: positives = all slots but 1 and 5, negatives (0, 3) and (2, 4)
    src, dst = rewritten_edges(ei, 5)
    conv.train()
    conv.p = 0.0
    choices = {"src": src, "dst": dst, "pos": torch.tensor([1, 0, 1, 1, 1, 0, 1, 1], dtype=torch.bool),
               "drop": torch.ones(8, 1, dtype=torch.bool), "neg": torch.tensor([[0, 2, 1], [3, 4, 1]]),
               "valid": torch.tensor([True, True, False])}
    out_t = conv(x, ei, choices)
    assert torch.allclose(out_t, out, atol=1e-12)
    assert abs(conv.att_loss.item() - 0.638262) < 1e-6
    # dropout: slot 0 dropped at p = 0.5 leaves target 1 with 2 * (alpha_1 x_2 + alpha_4 x_1)
    conv.p = 0.5
    choices["drop"] = torch.tensor([[0], [1], [1], [1], [1], [1], [1], [1]], dtype=torch.bool)
    out_d = conv(x, ei, choices)
    want_row1 = [2 * (0.346847 * 0.0 + 0.321826 * 0.5), 2 * (0.346847 * 2.0 + 0.321826 * -1.0)]
    assert torch.allclose(out_d[1], torch.tensor(want_row1, dtype=torch.float64), atol=1e-5)


def test_registry_and_defaults():
    from rgb_experiment_amd.initial_params import InitialParameters
    from rgb_experiment_amd.models import MODELS, REGISTRY, SuperGAT
    assert MODELS["supergat"] is SuperGAT and "supergat" not in REGISTRY
    assert InitialParameters.defaults_for("SuperGAT") == {
        "hidden_dim": 8, "heads": 8, "dropout_rate": 0.6, "edge_sample_ratio": 0.8, "neg_sample_ratio": 0.5}
    assert InitialParameters.model_names[:11] == ["MLP", "GCN", "GraphSAGE", "GAT", "APPNPStack", "GraphSAGE2", "PTA",
                                                   "DAGNN", "SGC", "GIN", "GGNN"]
    assert InitialParameters.model_names[11] == "SuperGAT"


def test_module_layout_and_strict_loading():
    from rgb_experiment_amd.models import SuperGAT
    from rgb_experiment_amd.nn import SuperGATConv
    model = SuperGAT(input_dim=24, hidden_dim=8, output_dim=5, heads=8, dropout_rate=0.6, edge_sample_ratio=0.8,
                     neg_sample_ratio=0.5)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert shapes == {"conv1.lin.weight": (64, 24), "conv1.att_l": (1, 8, 8), "conv1.att_r": (1, 8, 8), "conv1.bias": (64,),
                      "conv2.lin.weight": (40, 64), "conv2.att_l": (1, 8, 5), "conv2.att_r": (1, 8, 5), "conv2.bias": (5,)}
    assert isinstance(model.conv1, SuperGATConv) and not model.conv2.concat
    assert model.conv1.bias.abs().max().item() == 0.0  # zeros; the others glorot (inside their bound)
    assert model.conv1.att_l.abs().max().item() <= (6.0 / 16) ** 0.5
    ref = RefSuperGAT(24, 8, 5, 8, 0.6)
    ref.load_state_dict({k: v.double() for k, v in model.state_dict().items()}, strict=True)
    model.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)


def test_refusals():
    import rgb_experiment_amd as R
    from rgb_experiment_amd.nn import SuperGATConv
    g = torch.Generator().manual_seed(0)
    data = R.Data(x=torch.randn(30, 6, generator=g), y=torch.randint(0, 3, (30,), generator=g),
                  edge_index=torch.randint(0, 30, (2, 90), generator=g))
    params = R.InitialParameters.defaults_for("SuperGAT")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.experiment(params, specify_data=True, data=data, model_name="supergat", use_cpu=True, print_print=False)
    with pytest.raises(NotImplementedError):
        R.experiment(params, specify_data=True, data=data, model_name="FAGCN", use_cpu=True, print_print=False)
    with pytest.raises(NotImplementedError, match="SD"):
        SuperGATConv(4, 4, attention_type="SD")
    with pytest.raises(NotImplementedError, match="add_self_loops"):
        SuperGATConv(4, 4, add_self_loops=False)
    conv = SuperGATConv(4, 3, heads=2)
    with pytest.raises(RuntimeError, match="no CPU fallback|No CPU fallback|HIP"):
        conv(torch.randn(5, 4), torch.tensor([[0, 1], [1, 2]]))
    with pytest.raises(RuntimeError, match="no forward"):
        SuperGATConv(4, 3).get_attention_loss()


NEW_ENTRIES = ("rgbx_supergat_supported", "rgbx_supergat_loss_records", "rgbx_supergat_aggregate_fwd_f32",
               "rgbx_supergat_bwd_dst_f32", "rgbx_supergat_bwd_src_f32", "rgbx_supergat_sample_negatives",
               "rgbx_supergat_neg_loss_fwd_f32", "rgbx_supergat_neg_loss_bwd_f32", "rgbx_supergat_draws_u8")


def test_abi_declares_and_exports_the_new_entries():
    import ctypes
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
    p = 0x10000
    # widths: what GATConv.kernel_channels leaves unpadded
    ok = lib.rgbx_supergat_supported
    assert ok(8, 8) and ok(8, 40) and ok(1, 7) and ok(2, 64) and ok(1, 128) and ok(1, 256)
    assert not ok(1, 67) and not ok(1, 130) and not ok(1, 260) and not ok(0, 8)
    # host-side validation: every rejected call returns before a launch
    fwd = lambda **kw: lib.rgbx_supergat_aggregate_fwd_f32(
        kw.get("rowptr", p), p, p, kw.get("ldh", 64), p, p, None, p, 64, p, p, 10, 8, kw.get("C", 8), 0.2,
        kw.get("seed"), kw.get("p_drop", 0.6), 0.8, kw.get("rec"), kw.get("n_rec", 0), kw.get("stats"), None, None)
    assert fwd(rowptr=None) == -1 and b"null" in lib.rgbx_last_error_string()
    assert fwd(ldh=32) == -1
    assert fwd(seed=p) == -1                                    # training mode without loss buffers
    assert fwd(seed=p, rec=p, stats=p, n_rec=1) == -4           # too few loss records
    assert fwd(seed=p, rec=p, stats=p, n_rec=64, p_drop=1.0) == -1
    assert lib.rgbx_supergat_aggregate_fwd_f32(p, p, p, 1000, p, p, None, p, 1000, p, p, 10, 1, 1000, 0.2, None, 0.0, 1.0,
                                               None, 0, None, None, None) == -5   # a head wider than 64 lanes x 4 floats
    cnt = ctypes.c_int64(0)
    assert lib.rgbx_supergat_loss_records(1000, None, ctypes.byref(cnt)) == 0 and cnt.value == 250
    assert lib.rgbx_supergat_sample_negatives(p, 10, 1, p, 5, 8, p, p, None) == -1    # a pair needs two nodes
    assert lib.rgbx_supergat_sample_negatives(p, 10, 100, p, 0, 8, p, p, None) == 0   # nothing to do
    assert lib.rgbx_supergat_sample_negatives(p, 10, 100, None, 5, 8, p, p, None) == -1
    assert lib.rgbx_supergat_neg_loss_fwd_f32(p, 32, p, None, 5, 8, 8, p, 64, p, None) == -1   # leading dimension
    assert lib.rgbx_supergat_neg_loss_bwd_f32(p, 64, p, None, 5, 8, 8, None, p, 64, None) == -1
    assert lib.rgbx_supergat_bwd_dst_f32(p, p, p, 64, p, p, p, p, p, 64, None, p, 64, p + 4, p, 64, p, 10, 8, 8, 0.2, None,
                                         0.0, 1.0, None, None, None) == -3           # nodeq alignment
    assert lib.rgbx_supergat_bwd_src_f32(p, p, None, p, 64, p, p, p, 64, p, 64, p, 10, 8, 8, 0.2, p, 0.6, 0.8, p, None,
                                         None) == -1                                 # training mode without the slot map
    assert lib.rgbx_supergat_draws_u8(None, 5, 8, 0.6, 0.8, p, p, None) == -1
