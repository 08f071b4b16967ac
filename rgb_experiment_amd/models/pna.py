"""PNA — the zoo's two-ended stack (models/gine.py's conventions) with PyG's PNAConv (Corso et al., "Principal
Neighbourhood Aggregation for Graph Nets"): num_layers PNAConv layers, input_dim -> hidden_unit -> ... -> output_dim, with
ReLU and dropout between them and the log-softmax of the zoo's outputs behind the last. The hidden layers run `towers`
towers (hidden_unit must be a multiple), the last layer always one (the class count rarely divides). The degree
averages of the scalers are taken from the graph (PNAConv(deg=None)). With `edge_dim` every edge carries a feature row
(`edge_attr`, float32 [E, edge_dim]); without it the model runs on the node features alone. Not in the reference's zoo:
`model_name="pna"` is in MODELS only; `experiment(use_edge_attr=True)` passes data.edge_attr."""
import torch.nn as nn
import torch.nn.functional as F

from ..nn import PNAConv
from ._stack import model_output


class PNA(nn.Module):
    def __init__(self, input_dim, output_dim, hidden_unit, num_layers, dropout_rate,
                 aggregators=("mean", "max", "min", "std"), scalers=("identity", "amplification", "attenuation"), towers=1,
                 edge_dim=None, post_layers=1):
        super().__init__()
        if num_layers < 1:
            raise ValueError("num_layers must be at least 1")
        self.dropout_rate, self.edge_dim = dropout_rate, edge_dim
        dims = [input_dim] + [hidden_unit] * (num_layers - 1) + [output_dim]
        self.convs = nn.ModuleList(
            PNAConv(a, b, aggregators, scalers, deg=None, edge_dim=edge_dim, towers=towers if i + 2 < len(dims) else 1,
                    post_layers=post_layers)
            for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])))

    def forward(self, x, edge_index, edge_attr=None):
        if (edge_attr is None) != (self.edge_dim is None):
            raise ValueError(f"PNA: built with edge_dim={self.edge_dim}, called with"
                             f"{'out' if edge_attr is None else ''} edge_attr")
        for i, conv in enumerate(self.convs):
            x = conv(x, edge_index, edge_attr)
            if i + 1 < len(self.convs):
                x = F.relu(x)
                x = F.dropout(x, p=self.dropout_rate, training=self.training)
        return model_output(x)
