"""CGCNN — the zoo's encoder / decoder stack (models/gine.py's conventions) with PyG's CGConv (Xie & Grossman, "Crystal
Graph Convolutional Neural Networks for an Accurate and Interpretable Prediction of Material Properties"):
Linear(in, hid), then num_layers blocks CGConv(hid, edge_dim, aggr, batch_norm) -> ReLU -> dropout, then Linear(hid,
out). CGConv keeps its width (out_i = x_i + ...), hence the encoder in front and the decoder behind. With `edge_dim` > 0
every edge carries a feature row (`edge_attr`, float32 [E, edge_dim]); with 0 the model runs on the node features
alone. Not in the reference's zoo: `model_name="cgcnn"` is in MODELS only; `experiment(use_edge_attr=True)` passes
data.edge_attr."""
import torch.nn as nn
import torch.nn.functional as F

from ..nn import CGConv, Linear
from ._stack import model_output


class CGCNN(nn.Module):
    def __init__(self, input_dim, output_dim, hidden_unit, num_layers, dropout_rate, edge_dim=0, aggr="add",
                 batch_norm=True):
        super().__init__()
        if num_layers < 1:
            raise ValueError("num_layers must be at least 1")
        self.dropout_rate, self.edge_dim = dropout_rate, edge_dim
        self.encoder = Linear(input_dim, hidden_unit)
        self.convs = nn.ModuleList(CGConv(hidden_unit, edge_dim, aggr, batch_norm) for _ in range(num_layers))
        self.decoder = Linear(hidden_unit, output_dim)

    def forward(self, x, edge_index, edge_attr=None):
        x = self.encoder(x)
        for conv in self.convs:
            x = F.relu(conv(x, edge_index, edge_attr))
            x = F.dropout(x, p=self.dropout_rate, training=self.training)
        return model_output(self.decoder(x))
