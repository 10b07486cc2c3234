"""``optical_flow.operator`` drop-in (reference: optical_flow/operator/operator.py:8-165).

``warp`` runs on the gfx950 ``grid_warp`` kernel (the linspace base grid of ``warp_grid`` is fused into the
kernel, never materialised), registered as ``torch.ops.oflow.grid_warp`` with an autograd formula (frame and flow
gradients through ATen's grid_sampler_2d_backward on the same grid, optical_flow/_ops.py), so it traces under
torch.compile and differentiates in a photometric loss. The flow rescaling helpers are single elementwise passes and stay plain PyTorch
tensor ops, exactly as the reference writes them. Signatures, defaults, the asserts and
the quirks (Q8: ``warp`` is not the identity at zero flow with ``align_corners=False``; Q9: ``integrate`` passes
un-normalised flow to ``warp``) are the reference's.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch import Tensor
from torch.nn import functional as F

from .. import _native


def warp(
    frame: Tensor,
    flow: Tensor,
    mode: str = "bilinear",
    padding_mode: str = "border",
    align_corners: bool = False,
) -> Tensor:
    """Inverse warping with optical flow (`operator.py:8-33`).

    Args:
        frame: the image tensor of shape (B, C, H, W), on a ROCm GPU
        flow: the optical flow tensor of shape (B, 2, H, W), already normalized (see :func:`normalize`)
        mode: 'bilinear' | 'nearest' | 'bicubic' (grid_sample semantics)
        padding_mode: 'zeros' | 'border' | 'reflection'
        align_corners: grid_sample's ``align_corners``

    Returns:
        The warped image (B, C, H, W) fp32.
    """
    return _native.grid_warp(frame, flow, mode, padding_mode, align_corners)


def fb_consistency(
    flow_fw: Tensor,
    flow_bw: Tensor,
    alpha: float = 0.01,
    beta: float = 0.5,
    both: bool = False,
    return_error: bool = False,
):
    """Forward-backward consistency check of two flows in pixel units (an addition; the reference has none): the
    occlusion mask of UnFlow (Meister et al., AAAI 2018, their defaults). A pixel of ``flow_fw``'s frame is occluded when
    ``flow_bw``, sampled bilinearly where the pixel lands, does not cancel the pixel's own flow:
    ``|a + s|^2 > alpha * (|a|^2 + |s|^2) + beta``; a pixel that lands outside the frame, and any non-finite value,
    counts as occluded (include/oflow.h ``oflow_fb_consistency_f32`` states the arithmetic).

    Args:
        flow_fw: the flow frame 0 -> frame 1, (B, 2, H, W), channel 0 = x
        flow_bw: the flow frame 1 -> frame 0, same shape and device
        alpha, beta: the relative and absolute terms of the threshold
        both: also check ``flow_bw`` against ``flow_fw`` (the mask of frame 1), in the same kernel launch
        return_error: pair every mask with its squared residual ``|a + s|^2`` (fp32, +inf outside the frame)

    Returns:
        The bool mask (B, 1, H, W) of ``flow_fw``'s frame, True = occluded; with ``both`` the pair
        ``(mask_fw, mask_bw)``; with ``return_error`` every mask becomes ``(mask, error)``.

    GPU tensors run one kernel on the current stream (``torch.ops.oflow.fb_consistency``, no host sync); CPU tensors run
    the same arithmetic as a torch composition. There is no gradient: the inputs are detached.
    """
    what = "fb_consistency"
    for name, t in (("flow_fw", flow_fw), ("flow_bw", flow_bw)):
        if not isinstance(t, Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if not t.is_floating_point():
            raise TypeError(f"{what}: {name} must be a floating-point tensor, got {t.dtype}")
    if flow_fw.dim() != 4 or flow_fw.shape[1] != 2 or flow_fw.shape != flow_bw.shape:
        raise ValueError(f"{what}: flow_fw {tuple(flow_fw.shape)} and flow_bw {tuple(flow_bw.shape)} must be equal "
                         "(B, 2, H, W)")
    if flow_fw.device != flow_bw.device:
        raise ValueError(f"{what}: flow_fw and flow_bw are on different devices")
    fw, bw = flow_fw.detach(), flow_bw.detach()
    if fw.is_cuda:
        m_fw, m_bw, e_fw, e_bw = _native.fb_consistency(fw, bw, alpha, beta, both, return_error)
    else:
        fw, bw = fw.float().contiguous(), bw.float().contiguous()
        m_fw, e_fw = _fb_consistency_torch(fw, bw, float(alpha), float(beta))
        m_bw, e_bw = _fb_consistency_torch(bw, fw, float(alpha), float(beta)) if both else (None, None)
    first = (m_fw, e_fw) if return_error else m_fw
    if not both:
        return first
    return first, ((m_bw, e_bw) if return_error else m_bw)


def _fb_consistency_torch(a: Tensor, o: Tensor, alpha: float, beta: float) -> Tuple[Tensor, Tensor]:
    """One direction of ``fb_consistency`` on (B, 2, H, W) fp32 tensors in plain torch (the CPU path): the contract of
    include/oflow.h step by step, every product and sum a separate fp32 operation."""
    b, _, h, w = a.shape
    if a.numel() == 0:
        return a.new_zeros((b, 1, h, w), dtype=torch.bool), a.new_zeros((b, 1, h, w))
    u, v = a[:, 0], a[:, 1]
    px = torch.arange(w, dtype=torch.float32).view(1, 1, w) + u
    py = torch.arange(h, dtype=torch.float32).view(1, h, 1) + v
    inside = (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)
    pxs, pys = torch.where(inside, px, 0.0), torch.where(inside, py, 0.0)  # (outside: any valid tap, discarded below)
    fx, fy = torch.floor(pxs), torch.floor(pys)
    wx, wy = pxs - fx, pys - fy
    x0, y0 = fx.long(), fy.long()
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)

    def sample(plane: Tensor) -> Tensor:
        flat = plane.reshape(b, h * w)
        t00, t01 = flat.gather(1, (y0 * w + x0).view(b, -1)), flat.gather(1, (y0 * w + x1).view(b, -1))
        t10, t11 = flat.gather(1, (y1 * w + x0).view(b, -1)), flat.gather(1, (y1 * w + x1).view(b, -1))
        wxf, wyf = wx.reshape(b, -1), wy.reshape(b, -1)
        top = t00 + wxf * (t01 - t00)
        bot = t10 + wxf * (t11 - t10)
        return (top + wyf * (bot - top)).view(b, h, w)

    s0, s1 = sample(o[:, 0]), sample(o[:, 1])
    du, dv = u + s0, v + s1
    err = du * du + dv * dv
    thr = alpha * (u * u + v * v + s0 * s0 + s1 * s1) + beta
    mask = ~(err <= thr) | ~inside
    err = torch.where(inside, err, torch.full_like(err, float("inf")))
    return mask.unsqueeze(1), err.unsqueeze(1)


SPLAT_EPS = _native.SPLAT_EPS


def splat(
    frame: Tensor,
    flow: Tensor,
    metric: Optional[Tensor] = None,
    mode: str = "sum",
    return_weight: bool = False,
):
    """Forward warping (splatting) of a frame along a flow (an addition; the reference has none): summation, average,
    linear and softmax splatting of Niklaus and Liu (CVPR 2020). Every source pixel (x, y) is pushed to
    (x + u, y + v) and spread over the four pixels around that point with bilinear weights w;
    ``N_c(t) = sum w m frame_c`` and ``D(t) = sum w m`` over everything that reaches target t.

    Args:
        frame: (B, C, H, W)
        flow: (B, 2, H, W) in **pixel units**, channel 0 = x -- as :func:`fb_consistency` takes it, and not as
            :func:`warp` does (a normalized flow goes through :func:`denormalize` first)
        metric: the importance metric (B, 1, H, W) of the "linear" and "soft" modes, else None
        mode: the per-source weight m --
            "sum": m = 1, out = N (no normalisation);
            "avg": m = 1, out = N / (D + EPS);
            "linear": m = metric (expected >= 0), out = N / (D + EPS);
            "soft": m = exp(metric - max of metric over that image), out = N / (D + EPS);
            EPS = 1e-7
        return_weight: also return D as (B, 1, H, W) fp32, not differentiable; ``D == 0`` marks the holes

    Returns:
        out (B, C, H, W) fp32, or ``(out, D)``. A pixel that nothing reaches is exactly 0.

    A source whose landing point is non-finite, or has no tap inside the frame, contributes nothing; a tap outside the
    frame is dropped on its own. "soft" differs from the paper's unshifted form: the shift by the image's maximum keeps
    exp from overflowing and counts as a constant in the gradient, so EPS acts relative to the image's largest weight,
    and the returned D is in units of that largest weight. Non-finite frame or metric values make that image's output
    unspecified (include/oflow.h ``oflow_splat_f32`` states the arithmetic).

    GPU tensors run the native op on the current stream (``torch.ops.oflow.splat``, no host sync): 64-bit fixed-point
    sums, bit-identical from run to run and independent of the rest of the batch, with a native gather as the backward.
    CPU tensors run the same arithmetic as a torch composition with ``index_add_`` in float64, differentiable through
    autograd. Gradients flow to frame, flow and metric.
    """
    what = "splat"
    if mode not in _native.SPLAT_MODES:
        raise ValueError(f"{what}: unknown mode {mode!r} (one of {sorted(_native.SPLAT_MODES)})")
    needs_metric = mode in ("linear", "soft")
    if needs_metric and metric is None:
        raise ValueError(f"{what}: mode {mode!r} needs a metric")
    if not needs_metric and metric is not None:
        raise ValueError(f"{what}: mode {mode!r} takes no metric")
    for name, t in (("frame", frame), ("flow", flow)) + ((("metric", metric),) if needs_metric else ()):
        if not isinstance(t, Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if not t.is_floating_point():
            raise TypeError(f"{what}: {name} must be a floating-point tensor, got {t.dtype}")
    if frame.dim() != 4:
        raise ValueError(f"{what}: frame must be (B, C, H, W), got {tuple(frame.shape)}")
    b, _, h, w = frame.shape
    if tuple(flow.shape) != (b, 2, h, w):
        raise ValueError(f"{what}: flow must be (B, 2, H, W) = {(b, 2, h, w)}, got {tuple(flow.shape)}")
    if needs_metric and tuple(metric.shape) != (b, 1, h, w):
        raise ValueError(f"{what}: metric must be (B, 1, H, W) = {(b, 1, h, w)}, got {tuple(metric.shape)}")
    if flow.device != frame.device or (needs_metric and metric.device != frame.device):
        raise ValueError(f"{what}: all tensors must be on one device")
    if frame.is_cuda:
        out, weight = _native.splat(frame, flow, metric, mode)
    else:
        out, weight = _splat_torch(frame.float(), flow.float(), metric.float() if needs_metric else None, mode)
    return (out, weight) if return_weight else out


def _splat_torch(frame: Tensor, flow: Tensor, metric: Optional[Tensor], mode: str) -> Tuple[Tensor, Tensor]:
    """``splat`` on fp32 CPU tensors in plain torch: the contract of include/oflow.h with the sums taken in float64 by
    ``index_add_`` instead of in fixed point (the same values to within the fixed-point quantum), differentiable."""
    b, c, h, w = frame.shape
    hw = h * w
    if frame.numel() == 0 or hw == 0:
        return frame.new_zeros((b, c, h, w)), frame.new_zeros((b, 1, h, w))
    px = torch.arange(w, dtype=torch.float32).view(1, 1, w) + flow[:, 0]  # fp32 sums, rounded once
    py = torch.arange(h, dtype=torch.float32).view(1, h, 1) + flow[:, 1]
    keep = (px > -1) & (px < w) & (py > -1) & (py < h)  # False for NaN
    pxs, pys = torch.where(keep, px, 0.0), torch.where(keep, py, 0.0)
    x0f, y0f = torch.floor(pxs.detach()), torch.floor(pys.detach())
    fx, fy = pxs.double() - x0f.double(), pys.double() - y0f.double()  # exact in float64
    x0, y0 = x0f.long(), y0f.long()
    if mode == "linear":
        m = metric[:, 0].double()
    elif mode == "soft":
        m = torch.exp(metric[:, 0] - metric.detach().reshape(b, -1).amax(dim=1).view(b, 1, 1)).double()
    else:
        m = torch.ones((b, h, w), dtype=torch.float64)
    f64 = frame.double().permute(1, 0, 2, 3).reshape(c, b * hw)
    num = torch.zeros((c, b * hw), dtype=torch.float64)
    den = torch.zeros(b * hw, dtype=torch.float64)
    base = (torch.arange(b) * hw).view(b, 1, 1)
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            ok = keep & (x >= 0) & (x < w) & (y >= 0) & (y < h)
            wm = ((fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy)) * m
            wm = torch.where(ok, wm, torch.zeros_like(wm)).reshape(-1)  # a dropped tap adds 0 to pixel 0
            idx = (torch.where(ok, y * w + x, torch.zeros_like(x)) + base).reshape(-1)
            den = den.index_add(0, idx, wm)
            num = num.index_add(1, idx, wm * f64)
    out = num if mode == "sum" else num / (den + SPLAT_EPS)
    out = out.view(c, b, h, w).permute(1, 0, 2, 3).contiguous()
    return out.float(), den.detach().view(b, 1, h, w).float()


def interpolate_frame(
    frame0: Tensor,
    frame1: Tensor,
    flow_fw: Tensor,
    flow_bw: Tensor,
    t: float = 0.5,
    metric0: Optional[Tensor] = None,
    metric1: Optional[Tensor] = None,
) -> Tensor:
    """The frame at time t in [0, 1] between ``frame0`` (t = 0) and ``frame1`` (t = 1) by forward warping both:
    ``frame0`` is splatted along ``t * flow_fw`` and ``frame1`` along ``(1 - t) * flow_bw`` (flows in pixel units, as
    :func:`splat` takes them), "soft" with the metrics when both are given, else "avg", and the two are blended by
    their distance in time over the pixels each one reaches:
    ``((1 - t) h0 s0 + t h1 s1) / ((1 - t) h0 + t h1)`` with ``h = (D > 0)``; 0 where both have a hole.

    The usual metric is photometric consistency,
    ``metric0 = -alpha * (frame0 - warp(frame1, normalize(flow_fw))).abs().mean(1, keepdim=True)`` (and the mirror
    image for ``metric1``); ``alpha`` is the caller's to choose -- nothing here has tuned it.
    """
    if (metric0 is None) != (metric1 is None):
        raise ValueError("interpolate_frame: give both metrics or neither")
    mode = "avg" if metric0 is None else "soft"
    s0, d0 = splat(frame0, flow_fw * t, metric0, mode, return_weight=True)
    s1, d1 = splat(frame1, flow_bw * (1.0 - t), metric1, mode, return_weight=True)
    a0, a1 = (1.0 - t) * (d0 > 0).to(s0.dtype), t * (d1 > 0).to(s1.dtype)
    total = a0 + a1
    return (a0 * s0 + a1 * s1) / torch.where(total > 0, total, torch.ones_like(total))


def warp_grid(flow: Tensor) -> Tensor:
    """Sampling grid (B, H, W, 2) = linspace(-1, 1) base grid + normalized flow (B, H, W, 2)
    (`operator.py:36-56`). ``warp`` does not call this: its kernel forms the same grid in registers."""
    b, h, w, _ = flow.shape
    range_x = torch.linspace(-1.0, 1.0, w, device=flow.device)
    range_y = torch.linspace(-1.0, 1.0, h, device=flow.device)
    grid_y, grid_x = torch.meshgrid(range_y, range_x, indexing="ij")
    grid = torch.stack((grid_x, grid_y), dim=-1).unsqueeze(0).repeat(b, 1, 1, 1)
    return grid + flow


def scale(flow: Tensor, factor: Union[float, Tuple[float, float]] = 1.0) -> Tensor:
    """Multiply the X component by factor[0] and Y by factor[1] (`operator.py:59-82`)."""
    assert flow.size(1) == 2
    if isinstance(factor, (float, int)):
        factor = (factor, factor)
    assert len(factor) == 2
    scale_w = torch.empty_like(flow[:, 0]).fill_(factor[0])
    scale_h = torch.empty_like(flow[:, 0]).fill_(factor[1])
    return flow * torch.stack((scale_w, scale_h), dim=1)


def resize(
    flow: Tensor,
    size: Optional[Tuple[int, int]] = None,
    scale_factor: Optional[float] = None,
    mode: str = "bilinear",
) -> Tensor:
    """Spatially resize a flow map and rescale its vectors accordingly (`operator.py:85-114`)."""
    assert flow.size(1) == 2
    assert flow.ndimension() == 4
    _, _, h, w = flow.shape
    if scale_factor:
        size = (round(h * scale_factor), round(w * scale_factor))
    sy = size[0] / h
    sx = size[1] / w
    resized = F.interpolate(flow, size, mode=mode)
    return scale(resized, (sx, sy))


def normalize(flow: Tensor) -> Tensor:
    """Pixel units -> [-1, 1] grid units (`operator.py:117-130`)."""
    assert flow.size(1) == 2
    h, w = flow.shape[-2:]
    return scale(flow, (2.0 / max(w - 1, 1), 2.0 / max(h - 1, 1)))


def denormalize(flow: Tensor) -> Tensor:
    """[-1, 1] grid units -> pixel units (`operator.py:133-146`)."""
    assert flow.size(1) == 2
    h, w = flow.shape[-2:]
    return scale(flow, (max(w - 1, 1) / 2, max(h - 1, 1) / 2))


def integrate(*flows: Tensor) -> Tensor:
    """Chain flows f_0..f_k into one map: total = f_i + warp(total, f_i) from the back (`operator.py:149-165`)."""
    assert len(flows) >= 2
    total = flows[-1]
    for flow in reversed(flows[:-1]):
        assert flow.shape == total.shape, "All flows must have the same size."
        total = flow + warp(total, flow)
    return total
