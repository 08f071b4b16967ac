"""GATv2 — the stack of reference models/gat.py:5-32 with PyG's GATv2Conv in GATConv's place: GATv2Conv(in, hid, heads)
..., GATv2Conv(hid*heads, out, 1, concat=False), BatchNorm1d(hid*heads) between layers. `att_dropout` is the layers'
dropout on the attention coefficients (PyG's `dropout`); `dropout_rate` is stored and unused, as in every stack."""
from ..nn import GATv2Conv
from ._stack import ConvStack


class GATv2(ConvStack):
    def __init__(self, num_layers, hidden_unit, input_dim, output_dim, dropout_rate, heads, share_weights=False,
                 att_dropout=0.0):
        wide = hidden_unit * heads
        widths = [input_dim] + [wide] * (num_layers - 1) + [output_dim]
        kw = dict(share_weights=share_weights, dropout=att_dropout)

        def make(i, fan_in, fan_out):
            if i == num_layers - 1:
                return GATv2Conv(fan_in, output_dim, 1, concat=False, **kw)
            return GATv2Conv(fan_in, hidden_unit, heads, **kw)

        super().__init__(num_layers, dropout_rate, widths, make, wide)
        self.heads = heads
