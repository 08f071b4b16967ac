"""GraphSAGE — reference models/graphsage.py:6-32, built on the in-repo my_SAGEConv (:36-62)."""
from ..nn import MySAGEConv
from ._stack import ConvStack

my_SAGEConv = MySAGEConv  # the reference's class name


class GraphSAGE(ConvStack):
    """`aggr` ('mean' | 'max' | 'min' | 'add' | 'sum' | 'std' | 'var') goes to every conv: the keyword my_SAGEConv leaves to
    its caller (models/graphsage.py:38-40). It reaches this constructor through experiment()'s model_init_param. A list
    of aggregators is refused (ValueError): my_SAGEConv has no projection for their concatenation; GraphSAGE2 takes one.
    `gather_dtype` (None | torch.bfloat16 | 'bf16' | 'bfloat16') goes to every conv as well (nn.MySAGEConv)."""

    def __init__(self, num_layers, hidden_unit, input_dim, output_dim, dropout_rate, aggr="mean", gather_dtype=None):
        widths = [input_dim] + [hidden_unit] * (num_layers - 1) + [output_dim]
        super().__init__(num_layers, dropout_rate, widths,
                         lambda i, a, b: MySAGEConv(a, b, aggr=aggr, gather_dtype=gather_dtype), hidden_unit)
