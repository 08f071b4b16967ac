"""GGNN on the host: registry, defaults, module layout (reference names, strict state_dict loading), the refusal of
use_cpu=True, and host-side validation of the GRU entry points. No GPU needed."""
import math

import pytest
import torch
import torch.nn as nn


class RefGatedGraphConv(nn.Module):
    """float64 restatement of PyG GatedGraphConv (aggr='add'): same parameter names."""

    def __init__(self, C, L):
        super().__init__()
        self.C, self.L = C, L
        self.weight = nn.Parameter(torch.empty(L, C, C, dtype=torch.float64).uniform_(-1 / math.sqrt(C), 1 / math.sqrt(C)))
        self.rnn = nn.GRUCell(C, C).double()

    def forward(self, x, ei):
        if x.size(1) < self.C:
            x = torch.cat([x, x.new_zeros(x.size(0), self.C - x.size(1))], 1)
        src, dst = ei[0], ei[1]
        C = self.C
        for i in range(self.L):
            m = x @ self.weight[i]
            agg = torch.zeros_like(x).index_add_(0, dst, m[src])
            gi = agg @ self.rnn.weight_ih.t() + self.rnn.bias_ih
            gh = x @ self.rnn.weight_hh.t() + self.rnn.bias_hh
            r = torch.sigmoid(gi[:, :C] + gh[:, :C])
            z = torch.sigmoid(gi[:, C:2 * C] + gh[:, C:2 * C])
            n = torch.tanh(gi[:, 2 * C:] + r * gh[:, 2 * C:])
            x = (1 - z) * n + z * x
        return x


class RefGGNN(nn.Module):
    """float64 restatement of reference models/ggnn.py with the same submodule names."""

    def __init__(self, num_layers, hidden_unit, input_dim, output_dim):
        super().__init__()
        self.lin1 = nn.Linear(input_dim, hidden_unit).double()
        self.bn1 = nn.BatchNorm1d(hidden_unit).double()
        self.conv = RefGatedGraphConv(hidden_unit, num_layers)
        self.bn2 = nn.BatchNorm1d(hidden_unit).double()
        self.lin2 = nn.Linear(hidden_unit, output_dim).double()

    def forward(self, x, ei):
        x = self.lin2(self.bn2(self.conv(self.bn1(self.lin1(x)), ei)))
        return {"out": torch.log_softmax(x, 1), "emb": x}


def test_ggnn_is_dispatched_with_the_reference_defaults():
    from rgb_experiment_amd import InitialParameters
    from rgb_experiment_amd.models import GGNN, MODELS, REGISTRY
    assert MODELS["ggnn"] is GGNN
    assert all(MODELS[k] is v for k, v in REGISTRY.items())
    assert InitialParameters.defaults_for("ggnn") == {"num_layers": 2, "hidden_unit": 64, "dropout_rate": 0.5}
    assert InitialParameters.defaults_for("GGNN") == InitialParameters.defaults_for("ggnn")
    # appended: the earlier models keep their entries
    assert InitialParameters.model_names[:10] == ["MLP", "GCN", "GraphSAGE", "GAT", "APPNPStack", "GraphSAGE2", "PTA",
                                                  "DAGNN", "SGC", "GIN"]


def test_ggnn_layout_matches_the_reference_and_loads_its_state_dict():
    from rgb_experiment_amd.models import GGNN
    from rgb_experiment_amd.nn import GatedGraphConv
    torch.manual_seed(0)
    m = GGNN(num_layers=3, hidden_unit=16, input_dim=10, output_dim=4, dropout_rate=0.5)
    assert [n for n, _ in m.named_children()] == ["lin1", "bn1", "conv", "bn2", "lin2"]
    assert isinstance(m.conv, GatedGraphConv)
    shapes = {k: tuple(v.shape) for k, v in m.named_parameters()}
    assert shapes["conv.weight"] == (3, 16, 16)
    assert shapes["conv.rnn.weight_ih"] == (48, 16) and shapes["conv.rnn.weight_hh"] == (48, 16)
    assert shapes["conv.rnn.bias_ih"] == (48,) and shapes["conv.rnn.bias_hh"] == (48,)
    bound = 1 / math.sqrt(16)
    assert m.conv.weight.abs().max().item() <= bound  # PyG's uniform(C, weight)
    ref = RefGGNN(3, 16, 10, 4)
    assert sorted(ref.state_dict()) == sorted(m.state_dict())
    m.load_state_dict(ref.state_dict(), strict=True)
    assert torch.equal(m.conv.weight.detach(), ref.conv.weight.detach().float())
    assert torch.equal(m.conv.rnn.bias_hh.detach(), ref.conv.rnn.bias_hh.detach().float())


def test_gated_graph_conv_refuses_wider_inputs_and_other_aggregations():
    from rgb_experiment_amd.nn import GatedGraphConv
    conv = GatedGraphConv(8, 2)
    with pytest.raises(ValueError, match="input channels"):
        conv(torch.zeros(5, 9), torch.zeros(2, 0, dtype=torch.long))
    with pytest.raises(NotImplementedError):
        GatedGraphConv(8, 2, aggr="mean")


def test_gru_operands_restate_the_gru_cell():
    """pre = (A x) Weffᵀ + x Wrootᵀ + bias gives GRUCell's gate inputs (float64, A = identity, padded width)."""
    from rgb_experiment_amd import ops
    torch.manual_seed(1)
    C, Cp, N = 7, 8, 5
    cell = nn.GRUCell(C, C).double()
    W = torch.randn(C, C, dtype=torch.float64)
    x = torch.randn(N, C, dtype=torch.float64)
    weff, wroot, b = ops.gru_operands(W, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh, Cp)
    assert weff.shape == (4 * Cp, Cp) and wroot.shape == (4 * Cp, Cp) and b.shape == (4 * Cp,)
    xp = torch.nn.functional.pad(x, (0, Cp - C))
    pre = xp @ weff.t() + xp @ wroot.t() + b
    r, z = torch.sigmoid(pre[:, :Cp]), torch.sigmoid(pre[:, Cp:2 * Cp])
    n = torch.tanh(pre[:, 2 * Cp:3 * Cp] + r * pre[:, 3 * Cp:])
    got = ((1 - z) * n + z * xp)[:, :C]
    want = cell(x @ W, x)
    assert torch.allclose(got, want, atol=1e-12)


def test_experiment_refuses_ggnn_on_the_cpu():
    import rgb_experiment_amd as R
    g = torch.Generator().manual_seed(0)
    data = R.Data(x=torch.randn(60, 6, generator=g), y=torch.randint(0, 3, (60,), generator=g),
                  edge_index=torch.randint(0, 60, (2, 200), generator=g))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.experiment(R.InitialParameters.defaults_for("ggnn"), specify_data=True, data=data, model_name="ggnn",
                     use_cpu=True, print_print=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.experiment(R.InitialParameters.defaults_for("ggnn"), specify_data=True, data=data, model_name="GGNN",
                     use_cpu=True, print_print=False)


def test_gru_entry_points_validate_on_the_host():
    from rgb_experiment_amd import _lib
    lib = _lib.load()
    p = 0x10000  # 16-byte aligned, non-null, never dereferenced
    ok = lib.rgbx_gru_step_supported
    assert ok(8) and ok(32) and ok(40) and ok(64)
    assert not ok(4) and not ok(12) and not ok(96) and not ok(128) and not ok(0)
    step = lambda C, x=p, ldx=None, rowptr=p, out=p + 4096, pre=None, ldp=0: lib.rgbx_gru_step_f32(
        rowptr, p, x, C if ldx is None else ldx, p, p, p, out, C, None, C, pre, ldp, 10, C, None, None)
    assert step(64, rowptr=None) == -1 and b"null" in lib.rgbx_last_error_string()
    assert step(64, out=None) == -1
    assert step(96) == -5 and step(4) == -5                        # RGBX_E_SHAPE: the fused form's widths only
    assert step(64, x=p + 4) == -3                                  # RGBX_E_ALIGN
    assert step(64, ldx=32) == -1                                   # leading dimension < C
    assert step(64, pre=p, ldp=128) == -1                           # pre needs ld >= 4 C
    assert step(64, pre=p + 8, ldp=256) == -3
    assert step(64, out=p) == -1                                    # out aliases x
    fwd = lib.rgbx_gru_gate_fwd_f32
    assert fwd(None, 16, p, 4, p, 4, 10, 4, None) == -1
    assert fwd(p, 16, p, 4, p, 4, 10, 6, None) == -5                # C % 4
    assert fwd(p + 4, 16, p, 4, p, 4, 10, 4, None) == -3
    assert fwd(p, 12, p, 4, p, 4, 10, 4, None) == -1                # ldp < 4 C
    assert fwd(p, 16, p, 4, p, 4, -1, 4, None) == -1
    bwd = lib.rgbx_gru_gate_bwd_f32
    assert bwd(p, 16, p, 4, p, 4, None, 16, p, 4, 10, 4, None) == -1
    assert bwd(p, 16, p, 4, p, 4, p, 16, p + 4, 4, 10, 4, None) == -3
    assert bwd(p, 16, p, 4, p, 6, p, 16, p, 4, 10, 4, None) == -3  # ld % 4
    assert bwd(p, 16, p, 4, p, 4, p, 16, p, 4, 10, 10, None) == -5
    assert fwd(p, 16, p, 4, p, 4, 0, 4, None) == 0                   # nothing to do: no launch
