"""DeeperGCN (Li et al., "DeeperGCN: All You Need to Train Deeper GCNs") with PyG's GENConv and the softmax aggregator:
node_encoder = Linear(in, hid); h = convs[0](h); for l >= 1 the pre-activation residual block ("res+")
h = h + convs[l](dropout(relu(norms[l-1](h)))); logits = lin(dropout(relu(norms[L-1](h)))). `conv_kw` (t, learn_t,
per_channel_t, eps, expansion, bias) goes to every GENConv; `num_layers` is the depth of the stack, so the layers' MLPs keep
GENConv's default depth of 2. Unlike the reference's conv
stacks, where `dropout_rate` is stored and unused (models/gcn.py:15,25-31), it IS applied here (ops.dropout): the
architecture is defined with it. Not in the reference's zoo: `model_name="deepergcn"` is in MODELS only."""
import torch
import torch.nn as nn

from .. import ops
from ..nn import BatchNorm1d, GENConv, Linear
from ._stack import model_output


class DeeperGCN(nn.Module):
    def __init__(self, num_layers, hidden_unit, input_dim, output_dim, dropout_rate, **conv_kw):
        super().__init__()
        if num_layers < 1:
            raise ValueError("num_layers must be at least 1")
        self.num_layers = num_layers
        self.dropout_rate = dropout_rate
        self.node_encoder = Linear(input_dim, hidden_unit)
        self.convs = nn.ModuleList(GENConv(hidden_unit, hidden_unit, **conv_kw) for _ in range(num_layers))
        self.norms = nn.ModuleList(BatchNorm1d(hidden_unit) for _ in range(num_layers))
        self.lin = Linear(hidden_unit, output_dim)

    def _act(self, norm, h):
        return ops.dropout(torch.relu(norm(h)), self.dropout_rate, self.training)

    def forward(self, x, edge_index):
        h = self.node_encoder(x)
        h = self.convs[0](h, edge_index)
        for l in range(1, self.num_layers):
            h = h + self.convs[l](self._act(self.norms[l - 1], h), edge_index)
        return model_output(self.lin(self._act(self.norms[-1], h)))
