"""ResGatedGCN — the stack of models/gcn.py with PyG's ResGatedGraphConv (Bresson & Laurent's residual gated graph
convolution, the benchmarking literature's GatedGCN) in GCNConv's place: ResGatedGraphConv(in, hid) ...,
ResGatedGraphConv(hid, out), BatchNorm1d(hid) between layers, no activation. `root_weight` / `bias` go to every layer;
`dropout_rate` is stored and unused, as in every stack. Like GATv2 and GraphTransformer the model has no row in
InitialParameters: its `model_init_param` is the caller's (num_layers, hidden_unit, dropout_rate at the least)."""
from ..nn import ResGatedGraphConv
from ._stack import ConvStack


class ResGatedGCN(ConvStack):
    def __init__(self, num_layers, hidden_unit, input_dim, output_dim, dropout_rate, **conv_kw):
        widths = [input_dim] + [hidden_unit] * (num_layers - 1) + [output_dim]
        super().__init__(num_layers, dropout_rate, widths, lambda i, a, b: ResGatedGraphConv(a, b, **conv_kw), hidden_unit)
