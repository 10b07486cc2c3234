"""``smoothness_loss``: the edge-aware smoothness term (include/oflow.h ``oflow_smoothness_loss_f32`` states the
contract)."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _native

ORDERS = (1, 2)


def smoothness_loss(
    flow: Tensor,
    image: Tensor,
    order: int = 1,
    edge_weight: float = 150.0,
    image_range: float = 255.0,
) -> Tensor:
    """The edge-aware first- or second-order smoothness of a flow (an addition; the reference has none): the
    regulariser that accompanies the census loss in UFlow (Jonschkowski et al., ECCV 2020). None of the constants
    (150, 0.001) has been tuned here: they are the published ones.

    ``flow`` is (B, 2, H, W) in pixel units. ``image`` is (B, C, H, W).

    - Order 1: ``Dx f = f(x+1) - f(x)``;
      ``wx = exp(-(edge_weight / image_range) * mean_c |I_c(x+1) - I_c(x)|)``;
      ``Lx = mean over (B, 2, H, W-1) of wx * sqrt((Dx f)^2 + 0.001^2)``; ``Ly`` is the mirror image in y;
      ``loss = (Lx + Ly) / 2``.
    - Order 2: ``Dxx f = f(x+2) - 2 f(x+1) + f(x)``; ``wx`` is formed from ``I(x+2) - I(x)``; the mean is over
      (B, 2, H, W-2). ``Ly`` is the mirror image.
    - A direction whose domain is empty contributes 0.
    - The gradient goes to ``flow`` only. The image is data and gets none.

    Returns a 0-dim fp32 tensor on the inputs' device with no host synchronisation. GPU tensors run the native op on the
    current stream (``torch.ops.oflow.smoothness_loss``), bit-identical from run to run in both directions. CPU tensors
    run the same arithmetic as a differentiable torch composition, in fp32 -- or, when the flow is float64, in float64
    with a float64 result, which is what ``torch.autograd.gradcheck`` needs.
    """
    what = "smoothness_loss"
    for name, t in (("flow", flow), ("image", image)):
        if not isinstance(t, Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if not t.is_floating_point():
            raise TypeError(f"{what}: {name} must be a floating-point tensor, got {t.dtype}")
    if image.dim() != 4:
        raise ValueError(f"{what}: image must be (B, C, H, W), got {tuple(image.shape)}")
    b, _, h, w = image.shape
    if tuple(flow.shape) != (b, 2, h, w):
        raise ValueError(f"{what}: flow must be (B, 2, H, W) = {(b, 2, h, w)}, got {tuple(flow.shape)}")
    if flow.device != image.device:
        raise ValueError(f"{what}: all tensors must be on one device")
    if isinstance(order, bool) or not isinstance(order, int):
        raise TypeError(f"{what}: order must be an int, got {type(order).__name__}")
    if order not in ORDERS:
        raise ValueError(f"{what}: order must be one of {ORDERS}, got {order!r}")
    if not 0.0 < float(image_range) < float("inf"):
        raise ValueError(f"{what}: image_range must be a positive finite number, got {image_range!r}")
    if not -float("inf") < float(edge_weight) < float("inf"):
        raise ValueError(f"{what}: edge_weight must be a finite number, got {edge_weight!r}")
    if flow.is_cuda:
        return _native.smoothness_loss(flow, image, order, edge_weight, image_range)
    dtype = torch.float64 if flow.dtype == torch.float64 else torch.float32
    return smoothness_loss_torch(flow.to(dtype), image.detach().to(dtype), order, float(edge_weight), float(image_range))


def smoothness_loss_torch(flow: Tensor, image: Tensor, order: int, edge_weight: float, image_range: float) -> Tensor:
    """``smoothness_loss`` as a plain torch composition in the flow's dtype (the CPU path; on a GPU it is the ATen
    baseline the native op is measured against): the contract step by step, the two sums in float64."""
    k = edge_weight / image_range

    def direction(dim: int) -> Tensor:
        n = flow.shape[dim]
        if n <= order or flow.numel() == 0 or image.shape[1] == 0:
            return flow.sum() * 0.0 if flow.numel() else flow.new_zeros(())
        lo = lambda t, a: t.narrow(dim, a, n - order)  # noqa: E731
        # the flow differences in float64 (exact for fp32 flows), rounded once: near 0 the derivative of
        # sqrt(d^2 + 0.001^2) changes by 1 over a span of 0.001, so fp32 rounding inside the stencil would show
        f64 = flow.double()
        if order == 1:
            d = (lo(f64, 1) - lo(f64, 0)).to(flow.dtype)
        else:
            d = ((lo(f64, 2) - lo(f64, 1)) - (lo(f64, 1) - lo(f64, 0))).to(flow.dtype)
        edge = (lo(image, order) - lo(image, 0)).abs()
        mean = edge[:, 0]
        for c in range(1, image.shape[1]):  # channels in index order, as the kernel adds them
            mean = mean + edge[:, c]
        wgt = torch.exp(-k * (mean / image.shape[1])).unsqueeze(1)
        terms = wgt * torch.sqrt(d * d + 1e-6)
        return (terms.double().sum() / terms.numel()).to(flow.dtype)

    return (direction(3) + direction(2)) / 2
