"""GNN-FiLM — the stack of PyG's examples/film.py on FiLMConv (Brockschmidt, "GNN-FiLM: Graph Neural Networks with
Feature-wise Linear Modulation"): num_layers FiLMConv layers, input_dim -> hidden_unit -> ... -> output_dim, with
BatchNorm and dropout behind every layer but the last, which runs with act=None; the log-softmax of the zoo's outputs
behind it. With num_relations > 1 every edge carries a relation (`edge_type`, int64 [E] with values in
[0, num_relations)); with the default of one relation the model runs on ordinary graphs and takes no edge_type. The
aggregation runs in the rgbx_film_* kernels. Not in the reference's zoo: `model_name="film"` is in MODELS only;
`experiment(use_edge_type=True)` hands it data.edge_type."""
import torch.nn as nn
import torch.nn.functional as F

from ..nn import BatchNorm1d, FiLMConv
from ._stack import model_output


class FiLM(nn.Module):
    def __init__(self, input_dim, output_dim, hidden_unit, num_layers, dropout_rate, num_relations=1, aggr="mean"):
        super().__init__()
        if num_layers < 1:
            raise ValueError("num_layers must be at least 1")
        self.dropout_rate = dropout_rate
        dims = [input_dim] + [hidden_unit] * (num_layers - 1) + [output_dim]
        last = len(dims) - 2
        self.convs = nn.ModuleList(FiLMConv(a, b, num_relations, act=None if i == last else "relu", aggr=aggr)
                                   for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])))
        self.norms = nn.ModuleList(BatchNorm1d(hidden_unit) for _ in range(num_layers - 1))

    def forward(self, x, edge_index, edge_type=None):
        for conv, norm in zip(self.convs[:-1], self.norms):
            x = norm(conv(x, edge_index, edge_type))
            x = F.dropout(x, p=self.dropout_rate, training=self.training)
        return model_output(self.convs[-1](x, edge_index, edge_type))
