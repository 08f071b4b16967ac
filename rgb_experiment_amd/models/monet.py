"""MoNet — the zoo's two-ended stack (models/gine.py's conventions) with PyG's GMMConv (Monti et al., "Geometric deep
learning on graphs and manifolds using mixture model CNNs"): num_layers GMMConv layers, input_dim -> hidden_unit -> ... ->
output_dim, with ELU and dropout between them and the log-softmax of the zoo's outputs behind the last. Every edge carries
`dim` pseudo-coordinates (`edge_attr`, float32 [E, dim]); without them the model uses the paper's degree coordinates
(ops.degree_pseudo: 1 / sqrt(1 + indeg) of the source and of the target), which needs dim == 2. Not in the reference's
zoo: `model_name="monet"` is in MODELS only; `experiment(use_edge_attr=True)` passes data.edge_attr."""
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib, ops
from ..graph import LOOPS_KEEP, get_graph
from ..nn import GMMConv
from ._stack import model_output


class MoNet(nn.Module):
    def __init__(self, input_dim, output_dim, hidden_unit, num_layers, dropout_rate, kernel_size, dim=2):
        super().__init__()
        if num_layers < 1:
            raise ValueError("num_layers must be at least 1")
        self.dropout_rate, self.dim = dropout_rate, dim
        dims = [input_dim] + [hidden_unit] * (num_layers - 1) + [output_dim]
        self.convs = nn.ModuleList(GMMConv(a, b, dim, kernel_size) for a, b in zip(dims[:-1], dims[1:]))

    def forward(self, x, edge_index, edge_attr=None):
        if edge_attr is None and self.dim != 2:
            raise ValueError(f"MoNet: without edge_attr the degree pseudo-coordinates are used, which are 2 wide; this "
                             f"model was built with dim={self.dim}")
        e_slot = graph = None
        for i, conv in enumerate(self.convs):
            if edge_attr is not None:
                x = conv(x, edge_index, edge_attr)
            else:
                if graph is None:
                    _lib.require_device(x)
                    graph = get_graph(edge_index, x.size(0), LOOPS_KEEP)
                    e_slot = ops.degree_pseudo(graph)
                x = conv.forward_slots(x, graph, e_slot)
            if i + 1 < len(self.convs):
                x = F.elu(x)
                x = F.dropout(x, p=self.dropout_rate, training=self.training)
        return model_output(x)
