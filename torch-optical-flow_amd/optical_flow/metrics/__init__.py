"""``optical_flow.metrics`` (reference: optical_flow/metrics/__init__.py): the evaluation metrics of the reference with
the torchmetrics surface it uses, on one fused gfx950 reduction (csrc/flow_metrics.hip) for GPU tensors."""
from .epe import AverageEndPointError, end_point_error
from .f1 import OutlierRatio

__all__ = ["AverageEndPointError", "OutlierRatio", "end_point_error"]
