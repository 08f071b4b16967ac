"""RGCN — the zoo's two-ended stack (models/gine.py's conventions) with PyG's RGCNConv (Schlichtkrull et al., "Modeling
Relational Data with Graph Convolutional Networks"): num_layers RGCNConv layers, input_dim -> hidden_unit -> ... ->
output_dim, with ReLU and dropout between them and the log-softmax of the zoo's outputs behind the last. Every edge
carries a relation (`edge_type`, int64 [E] with values in [0, num_relations)); `num_bases` selects the basis
decomposition, whose aggregation runs in the rgbx_rgcn_mix_* kernels. Not in the reference's zoo: `model_name="rgcn"` is
in MODELS only and needs `experiment(use_edge_type=True)`."""
import torch.nn as nn
import torch.nn.functional as F

from ..nn import RGCNConv
from ._stack import model_output


class RGCN(nn.Module):
    def __init__(self, input_dim, output_dim, hidden_unit, num_layers, dropout_rate, num_relations, num_bases=None):
        super().__init__()
        if num_layers < 1:
            raise ValueError("num_layers must be at least 1")
        self.dropout_rate = dropout_rate
        dims = [input_dim] + [hidden_unit] * (num_layers - 1) + [output_dim]
        self.convs = nn.ModuleList(RGCNConv(a, b, num_relations, num_bases=num_bases)
                                   for a, b in zip(dims[:-1], dims[1:]))

    def forward(self, x, edge_index, edge_type):
        for i, conv in enumerate(self.convs):
            x = conv(x, edge_index, edge_type)
            if i + 1 < len(self.convs):
                x = F.relu(x)
                x = F.dropout(x, p=self.dropout_rate, training=self.training)
        return model_output(x)
