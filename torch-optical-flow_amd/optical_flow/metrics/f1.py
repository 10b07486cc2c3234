"""Outlier ratio (reference: optical_flow/metrics/f1.py)."""
from __future__ import annotations

from . import _stats


class OutlierRatio(_stats.FlowMetric):
    """Outlier ratio, also known as F1 (`f1.py:10-55`): the share of pixels whose end-point-error exceeds
    ``abs_threshold`` *and* whose error relative to the target's magnitude exceeds ``rel_threshold`` (both strict; a
    zero-magnitude target with an error above ``abs_threshold`` is an outlier, as ``inf > rel_threshold``).

    Args:
        dim: the dimension along which to compute the end-point-error (Euclidean distance)
        abs_threshold: the threshold of absolute error above which a pixel is considered an outlier
        rel_threshold: the threshold of relative error above which a pixel is considered an outlier
    """

    numerator = _stats.OUTLIERS

    def __init__(self, dim: int = 1, abs_threshold: float = 3.0, rel_threshold: float = 0.05) -> None:
        super().__init__(dim=dim, abs_threshold=abs_threshold, rel_threshold=rel_threshold)
