"""FAGCN — reference models/fagcn.py: dropout -> relu(t1) -> dropout -> raw; num_layers x FAConv(h, raw, edge_index);
t2. The layers share `raw`, the output of the first Linear, as their eps-weighted residual."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..nn import FAConv, Linear
from ._stack import model_output


class FAGCN(nn.Module):
    def __init__(self, num_layers, input_dim, hidden_unit, output_dim, dropout_rate, epsilon):
        super().__init__()
        self.eps, self.layer_num, self.dropout = epsilon, num_layers, dropout_rate
        self.layers = nn.ModuleList(FAConv(hidden_unit, epsilon, dropout_rate) for _ in range(num_layers))
        self.t1 = Linear(input_dim, hidden_unit)
        self.t2 = Linear(hidden_unit, output_dim)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_normal_(self.t1.weight, gain=1.414)
        nn.init.xavier_normal_(self.t2.weight, gain=1.414)

    def forward(self, x, edge_index):
        h = ops.dropout(x, self.dropout, self.training)  # features carried by their non-zeros stay on them
        h = torch.relu(self.t1(h))
        h = F.dropout(h, p=self.dropout, training=self.training)
        raw = h
        for layer in self.layers:
            h = layer(h, raw, edge_index)
        return model_output(self.t2(h))
