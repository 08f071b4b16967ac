"""GraphTransformer — the stack of models/gatv2.py with PyG's TransformerConv (scaled dot-product attention, UniMP) in
GATv2Conv's place: TransformerConv(in, hid, heads) ..., TransformerConv(hid*heads, out, 1, concat=False),
BatchNorm1d(hid*heads) between layers. `att_dropout` is the layers' dropout on the attention coefficients (PyG's
`dropout`), `beta` / `root_weight` their skip connection; `dropout_rate` is stored and unused, as in every stack."""
from ..nn import TransformerConv
from ._stack import ConvStack


class GraphTransformer(ConvStack):
    def __init__(self, num_layers, hidden_unit, input_dim, output_dim, dropout_rate, heads, att_dropout=0.0, beta=False,
                 root_weight=True):
        wide = hidden_unit * heads
        widths = [input_dim] + [wide] * (num_layers - 1) + [output_dim]
        kw = dict(dropout=att_dropout, beta=beta, root_weight=root_weight)

        def make(i, fan_in, fan_out):
            if i == num_layers - 1:
                return TransformerConv(fan_in, output_dim, 1, concat=False, **kw)
            return TransformerConv(fan_in, hidden_unit, heads, **kw)

        super().__init__(num_layers, dropout_rate, widths, make, wide)
        self.heads = heads
