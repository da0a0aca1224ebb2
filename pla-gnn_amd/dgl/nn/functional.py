"""dgl.nn.functional: edge_softmax, the same function as dgl.ops.edge_softmax."""
from ..ops import edge_softmax  # noqa: F401

__all__ = ["edge_softmax"]
