"""End-point error (reference: optical_flow/metrics/epe.py)."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _native
from . import _stats


class AverageEndPointError(_stats.FlowMetric):
    """Average End-to-end Point Error (AEPE or EPE for short): the mean 2-norm of the residual flow vectors
    (`epe.py:8-40`), optionally over the pixels with ``valid >= 0.5`` only. See :func:`end_point_error` for the
    functional form.

    Args:
        dim: the dimension along which to compute the end-point-error
    """

    numerator = _stats.SUM_EPE

    def __init__(self, dim: int = 1) -> None:
        super().__init__(dim=dim)


def end_point_error(pred: Tensor, target: Tensor, dim: int = 1, reduce: bool = True) -> Tensor:
    """End-to-end Point Error (`epe.py:43-65`): the 2-norm of ``pred - target`` along ``dim``; the mean over all
    vectors (a 0-dim tensor) by default, the per-vector errors (the shape without ``dim``) with ``reduce=False``.

    GPU tensors that need no gradient run the fused kernel: the map and the float64 sum in one pass. CPU tensors, and
    calls that autograd must differentiate, run the reference's torch composition."""
    if not _stats._native_ok(pred, target):
        epe = torch.norm(pred - target, p=2, dim=dim)
        return epe.mean() if reduce else epe
    p, t, _, reduced = _stats.as_b2hw(pred, target, None, dim)
    state = _stats.new_state(pred.device)
    epe_map = _native.ops().flow_error_stats(p, t, None, 0.0, 0.0, 0.0, state, not reduce)
    if reduce:
        return (state[_stats.SUM_EPE] / state[_stats.TOTAL]).to(pred.dtype if pred.is_floating_point() else torch.float32)
    return epe_map.reshape(reduced).to(pred.dtype if pred.is_floating_point() else torch.float32)
