"""dgl.nn — PyTorch backend only (the reference uses dgl.nn.pytorch, code/model.py:7)."""
from . import functional  # noqa: F401
from . import pytorch  # noqa: F401
from .pytorch import GATConv, GATv2Conv, GraphConv, SAGEConv  # noqa: F401
