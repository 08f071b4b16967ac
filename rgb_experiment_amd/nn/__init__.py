from .conv import GCNConv, SAGEConv, MySAGEConv, GATConv, APPNP, SGConv, GINConv, GINEConv, PNAConv, RGCNConv, FiLMConv, GMMConv, GatedGraphConv, SuperGATConv, GATv2Conv, TransformerConv, ResGatedGraphConv, CGConv, GENConv, FAConv
from .batchnorm import BatchNorm1d
from .linear import Linear
from .correct_and_smooth import CorrectAndSmooth, LabelPropagation

__all__ = ["GCNConv", "SAGEConv", "MySAGEConv", "GATConv", "APPNP", "SGConv", "GINConv", "GINEConv", "PNAConv", "RGCNConv", "FiLMConv", "GMMConv", "GatedGraphConv", "SuperGATConv", "GATv2Conv", "TransformerConv", "ResGatedGraphConv", "CGConv", "GENConv", "FAConv",
           "CorrectAndSmooth", "LabelPropagation", "BatchNorm1d", "Linear"]
