"""Checkpoint evaluation: the reference's validation loop (methods/raft/model/raft.py:183-196 under the Lightning
trainer) as a plain function over any iterable of batches. The Lightning CLI and the datasets stay out of scope.

Per batch ``RAFT.validation_step`` pads, runs the test-mode forward, unpads and updates ``epe_val`` / ``f1_val`` on the
device without a host synchronisation; the only device-to-host transfers are the two ``compute()`` results at the end.
Under one process per GPU (``torch.distributed`` initialised) every rank feeds its own batches and ``compute()`` sums
the metric states over the ranks, so each rank returns the metrics of the whole set.
"""
from __future__ import annotations

import os
import sys
from typing import Dict, Iterable, Tuple

import torch
from torch import Tensor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from model import RAFT  # noqa: E402


def validate(model: RAFT, batches: Iterable[Tuple[Tensor, Tensor, Tensor, Tensor]], stage: str = "sintel") -> Dict[str, float]:
    """EPE and F1 (outlier ratio, 3 px and 5 %) of ``model`` over ``batches`` of ``(img0, img1, flow_gt, valid)``;
    ``stage`` selects the padding ('sintel': symmetric, anything else: KITTI's). Tensors are moved to the device of the
    model's parameters. Returns ``{"epe_val": ..., "f1_val": ...}`` (NaN when no pixel was valid)."""
    device = next(model.parameters()).device
    was_training = model.training
    model.eval()
    model.epe_val.reset()
    model.f1_val.reset()
    try:
        with torch.inference_mode():
            for i, batch in enumerate(batches):
                model.validation_step(tuple(t.to(device, non_blocking=True) for t in batch), i, stage=stage)
            epe, f1 = model.epe_val.compute(), model.f1_val.compute()
    finally:
        model.train(was_training)
    return {"epe_val": float(epe), "f1_val": float(f1)}
