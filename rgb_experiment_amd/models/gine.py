"""GINE — models/gin.py's stack with PyG's GINEConv (GIN with a feature row per edge; Hu et al., "Strategies for
Pre-training Graph Neural Networks", the OGB baselines' layer) in GINConv's place: encoder = Linear(in, hid), then
num_layers blocks GINEConv(Linear-ReLU-Linear-ReLU-BatchNorm at hid, train_eps=True, edge_dim=edge_dim), then
lin1 -> ReLU -> dropout -> lin2. The node encoder is there because relu(x_j + e_ji) does not commute with GIN's
transform-first trick (models/gin.py's first block gathers at nn's output width): the message is formed at the width of
x, so every conv runs at hidden_unit. Not in the reference's zoo: `model_name="gine"` is in MODELS only."""
import torch.nn as nn
import torch.nn.functional as F

from ..nn import GINEConv, Linear
from ._stack import model_output
from .gin import _block


class GINE(nn.Module):
    def __init__(self, input_dim, output_dim, hidden_unit, num_layers, dropout_rate, edge_dim):
        super().__init__()
        if num_layers < 1:
            raise ValueError("num_layers must be at least 1")
        self.dropout_rate = dropout_rate
        self.encoder = Linear(input_dim, hidden_unit)
        self.convs = nn.ModuleList(GINEConv(_block(hidden_unit, hidden_unit), train_eps=True, edge_dim=edge_dim)
                                   for _ in range(num_layers))
        self.lin1 = Linear(hidden_unit, hidden_unit)
        self.lin2 = Linear(hidden_unit, output_dim)

    def forward(self, x, edge_index, edge_attr):
        x = self.encoder(x)
        for conv in self.convs:
            x = conv(x, edge_index, edge_attr)
        x = F.relu(self.lin1(x))
        x = F.dropout(x, p=self.dropout_rate, training=self.training)
        return model_output(self.lin2(x))
