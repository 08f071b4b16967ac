"""SuperGAT — reference models/supergat.py: dropout -> elu(SuperGATConv(in, hidden_dim, heads)) -> dropout ->
SuperGATConv(hidden_dim * heads, out, heads, concat=False); the forward also returns the sum of the two layers'
attention losses, which the training loop adds to the classification loss (itexperiments.py:431-432)."""
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..nn import SuperGATConv
from ._stack import ModelOutput


class SuperGATOutput(ModelOutput):
    """{'out', 'emb', 'x'} as every model returns them, plus 'att_loss'."""

    def __init__(self, logits, att_loss):
        super().__init__(logits)
        dict.__setitem__(self, "att_loss", att_loss)

    def keys(self):
        return super().keys() + ["att_loss"]

    def __len__(self):
        return 4


class SuperGAT(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, heads, dropout_rate, edge_sample_ratio, neg_sample_ratio):
        super().__init__()
        self.dropout_rate = dropout_rate
        kw = dict(dropout=dropout_rate, attention_type="MX", edge_sample_ratio=edge_sample_ratio,
                  neg_sample_ratio=neg_sample_ratio)
        self.conv1 = SuperGATConv(input_dim, hidden_dim, heads=heads, **kw)
        self.conv2 = SuperGATConv(hidden_dim * heads, output_dim, heads=heads, concat=False, **kw)

    def forward(self, x, edge_index):
        x = ops.dropout(x, self.dropout_rate, self.training)
        x = F.elu(self.conv1(x, edge_index))
        att_loss = self.conv1.get_attention_loss()
        x = F.dropout(x, p=self.dropout_rate, training=self.training)
        x = self.conv2(x, edge_index)
        att_loss = att_loss + self.conv2.get_attention_loss()
        return SuperGATOutput(x, att_loss)

    def masked_ce(self, x, edge_index, y, mask):
        """(loss, stats) of the masked cross-entropy of this model's logits, as ConvStack.masked_ce returns them; the
        attention loss of the same forward is kept in `self.att_loss` for the training loop."""
        res = self.forward(x, edge_index)
        self.att_loss = res["att_loss"]
        return ops.ce_from_logits(res["emb"], y, mask)
