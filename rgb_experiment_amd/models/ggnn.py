"""GGNN — reference models/ggnn.py:5-32: lin1 -> bn1 -> GatedGraphConv(hidden_unit, num_layers) -> bn2 -> lin2, no
activation and no dropout anywhere (the reference stores dropout_rate and never uses it)."""
import torch.nn as nn

from ..nn import BatchNorm1d, GatedGraphConv, Linear
from ._stack import model_output


class GGNN(nn.Module):
    def __init__(self, num_layers, hidden_unit, input_dim, output_dim, dropout_rate):
        super().__init__()
        self.num_layers = num_layers
        self.dropout_rate = dropout_rate
        self.lin1 = Linear(input_dim, hidden_unit)
        self.bn1 = BatchNorm1d(hidden_unit)
        self.conv = GatedGraphConv(hidden_unit, num_layers)
        self.bn2 = BatchNorm1d(hidden_unit)
        self.lin2 = Linear(hidden_unit, output_dim)

    def forward(self, x, edge_index):
        x = self.bn1(self.lin1(x))
        x = self.conv(x, edge_index)
        return model_output(self.lin2(self.bn2(x)))
