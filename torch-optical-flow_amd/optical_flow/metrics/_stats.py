"""Shared machinery of ``optical_flow.metrics``: the per-pixel flow error statistics behind every metric.

On ROCm GPU tensors the statistics come from ``torch.ops.oflow.flow_error_stats`` (csrc/flow_metrics.hip): one
streaming pass over pred / target / valid plus a one-workgroup finalize that adds

    {sum epe, n, n_outlier, n(epe < 1), n(epe < 3), n(epe < 5), 0, 0}        (float64)

into a device accumulator, with no host synchronisation. On CPU tensors the same eight numbers come from the
reference's torch composition (optical_flow/metrics/epe.py:24-65, f1.py:34-55).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from .. import _native

SUM_EPE, TOTAL, OUTLIERS, LT1, LT3, LT5 = range(6)
STATE_SIZE = 8  # the kernel's double[8] (include/oflow.h oflow_flow_error_stats_f32)


def new_state(device) -> Tensor:
    # never an inference tensor: a state created under torch.inference_mode() (validate) must stay updatable outside it
    with torch.inference_mode(False):
        return torch.zeros(STATE_SIZE, dtype=torch.float64, device=device)


def as_b2hw(pred: Tensor, target: Tensor, valid: Optional[Tensor], dim: int) -> Tuple[Tensor, Tensor, Optional[Tensor], Tuple[int, ...]]:
    """pred / target with the flow components along ``dim`` -> (B, 2, H, W) views where they already are 4-D with
    ``dim == 1`` (so that a cropped view stays a view), else ``movedim`` + reshape to (N, 2, 1, M) (may copy). ``valid``
    holds one element per flow vector, in the order of the reduced shape (the reference flattens it, epe.py:31).
    Returns the reduced shape (pred's shape without ``dim``) too."""
    if pred.shape != target.shape:
        raise RuntimeError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} must have the same shape")
    d = dim % pred.dim() if pred.dim() else 0
    if pred.dim() == 0 or pred.shape[d] != 2:
        raise ValueError(
            f"the native metrics kernel reduces 2-component flow vectors; dimension {dim} of {tuple(pred.shape)} "
            "does not have 2 entries")
    reduced = tuple(s for i, s in enumerate(pred.shape) if i != d)
    if pred.dim() == 4 and d == 1:
        p, t = pred, target
    else:
        p, t = pred.movedim(d, 0), target.movedim(d, 0)
        if p.dim() == 1:  # a single flow vector
            p, t = p.reshape(1, 2, 1, 1), t.reshape(1, 2, 1, 1)
        else:
            n, m = p.shape[1], 1
            for s in p.shape[2:]:
                m *= s
            p = p.reshape(2, n, 1, m).movedim(0, 1)
            t = t.reshape(2, n, 1, m).movedim(0, 1)
    if valid is not None:
        b, _, h, w = p.shape
        if valid.numel() != b * h * w:
            raise RuntimeError(f"valid {tuple(valid.shape)} must have one element per flow vector of {tuple(pred.shape)}")
        if tuple(valid.shape) != (b, h, w) and tuple(valid.shape) != (b, 1, h, w):
            valid = valid.reshape(b, h, w)
    return p, t, valid, reduced


def _native_ok(pred: Tensor, target: Tensor) -> bool:
    """The fused kernel runs on GPU tensors that need no gradient; a differentiable call (the EPE as a loss) and CPU
    tensors run the torch composition."""
    return pred.is_cuda and not (torch.is_grad_enabled() and (pred.requires_grad or target.requires_grad))


def accumulate(state: Tensor, pred: Tensor, target: Tensor, valid: Optional[Tensor], dim: int, abs_threshold: float,
               rel_threshold: float, max_flow: float = 0.0) -> None:
    """state[0:6] += the statistics of one batch (in place; two launches and no synchronisation on the GPU)."""
    if pred.is_cuda:
        p, t, v, _ = as_b2hw(pred.detach(), target.detach(), valid, dim)
        _native.ops().flow_error_stats(p, t, v, float(abs_threshold), float(rel_threshold), float(max_flow), state, False)
        return
    accumulate_torch(state, pred, target, valid, dim, abs_threshold, rel_threshold, max_flow)


def accumulate_torch(state: Tensor, pred: Tensor, target: Tensor, valid: Optional[Tensor], dim: int, abs_threshold: float,
                     rel_threshold: float, max_flow: float = 0.0) -> None:
    """``accumulate`` as the reference's torch composition (epe.py:29-37, f1.py:37-50), sums in float64: the CPU path
    (on GPU tensors the boolean index synchronises with the host: tools/exp/run_metrics_ab.py times it there)."""
    epe = torch.norm(pred.detach() - target.detach(), p=2, dim=dim).reshape(-1)
    mag = torch.norm(target.detach(), p=2, dim=dim).reshape(-1)
    outliers = (epe > abs_threshold) & ((epe / mag) > rel_threshold)
    if valid is not None:
        keep = valid.reshape(-1) >= 0.5
        if max_flow > 0 and max_flow != float("inf"):
            keep = keep & (mag < max_flow)
        epe, outliers = epe[keep], outliers[keep]
    elif max_flow > 0 and max_flow != float("inf"):
        keep = mag < max_flow
        epe, outliers = epe[keep], outliers[keep]
    batch = [epe.sum(dtype=torch.float64), epe.numel(), outliers.sum(), (epe < 1).sum(), (epe < 3).sum(), (epe < 5).sum()]
    state[:6] += torch.stack([torch.as_tensor(x, dtype=torch.float64) for x in batch]).to(state.device)


class FlowMetric(nn.Module):
    """The torchmetrics surface the reference's metrics use (torchmetrics itself is not required): ``update``,
    ``compute``, ``reset`` and ``forward`` (update, return the batch value). The state is one float64 vector on the
    device of the first update -- a plain attribute, neither buffer nor parameter, so ``state_dict()`` and
    ``.to()`` / ``.half()`` of an owning module leave it alone. Sums accumulate in float64 (the reference keeps a running
    fp32 sum). Under ``torch.distributed`` ``compute()`` sums the state over the ranks (``dist_reduce_fx="sum"``)."""

    numerator = SUM_EPE

    def __init__(self, dim: int = 1, abs_threshold: float = 3.0, rel_threshold: float = 0.05) -> None:
        super().__init__()
        self.dim = dim
        self.abs_threshold = abs_threshold
        self.rel_threshold = rel_threshold
        self._state: Optional[Tensor] = None

    def reset(self) -> None:
        if self._state is not None:
            self._state.zero_()

    def _state_on(self, device) -> Tensor:
        if self._state is None or self._state.device != device:
            new = new_state(device)
            if self._state is not None:
                new += self._state.to(device)
            self._state = new
        return self._state

    def update(self, pred: Tensor, target: Tensor, valid: Optional[Tensor] = None) -> None:
        accumulate(self._state_on(pred.device), pred, target, valid, self.dim, self.abs_threshold, self.rel_threshold)

    def _value(self, state: Tensor) -> Tensor:
        return (state[self.numerator] / state[TOTAL]).float()

    def forward(self, pred: Tensor, target: Tensor, valid: Optional[Tensor] = None) -> Tensor:
        batch = new_state(pred.device)
        accumulate(batch, pred, target, valid, self.dim, self.abs_threshold, self.rel_threshold)
        self._state_on(pred.device).add_(batch)
        return self._value(batch)

    def compute(self) -> Tensor:
        """The metric over everything seen since the last reset, a 0-dim fp32 tensor (NaN when nothing was selected)."""
        state = self._state
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized():
            if state is None:  # a rank that saw no batch still takes part in the reduction
                on_gpu = "nccl" in str(dist.get_backend()) and torch.cuda.is_available()
                state = new_state(torch.device("cuda", torch.cuda.current_device()) if on_gpu else "cpu")
            state = state.clone()
            dist.all_reduce(state)  # one float64 vector, summed
        elif state is None:
            state = new_state("cpu")
        return self._value(state)
