"""GraphSAGE2 — reference models/graphsage2.py:7-33 (PyG SAGEConv: aggregate first, then Linear)."""
from ..nn import SAGEConv
from ._stack import ConvStack


class GraphSAGE2(ConvStack):
    """`aggr` ('mean' | 'max' | 'min' | 'add' | 'sum' | 'std' | 'var', or a list of distinct ones such as
    ['mean', 'max', 'min', 'std']: PyG's MultiAggregation, one gather pass per layer) goes to every conv (PyG SAGEConv's
    keyword). `gather_dtype` (None | torch.bfloat16 | 'bf16' | 'bfloat16') goes to every conv as well (nn.SAGEConv)."""

    def __init__(self, num_layers, hidden_unit, input_dim, output_dim, dropout_rate, aggr="mean", gather_dtype=None):
        widths = [input_dim] + [hidden_unit] * (num_layers - 1) + [output_dim]
        super().__init__(num_layers, dropout_rate, widths,
                         lambda i, a, b: SAGEConv(a, b, aggr=aggr, gather_dtype=gather_dtype), hidden_unit)
