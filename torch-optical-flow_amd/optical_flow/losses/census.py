"""``census_loss``: the ternary census loss (include/oflow.h ``oflow_census_loss_f32`` states the contract)."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import _native

PATCHES = (3, 5, 7)


def census_loss(
    frame0: Tensor,
    frame1: Tensor,
    mask: Optional[Tensor] = None,
    patch: int = 7,
    image_range: float = 255.0,
    return_map: bool = False,
):
    """The ternary census loss between two frames over a ``patch`` x ``patch`` neighbourhood (an addition; the reference
    has none): the photometric term of UnFlow (Meister et al., AAAI 2018) and UFlow (Jonschkowski et al., ECCV 2020).
    None of the constants (0.81, 0.1, 0.01, 0.4) has been tuned here: they are the published ones.

    ``frame0`` and ``frame1`` are (B, C, H, W). In a training loss ``frame1`` is the second image already warped back.

    - Grey value: ``g = (sum_c frame_c) * 255 / (image_range * C)``.
    - Set ``r = patch // 2``. Interior pixels are those with ``r <= y < H - r`` and ``r <= x < W - r``.
    - For an interior pixel p and each of the ``patch^2 - 1`` offsets d != 0:
      ``delta_k = g_k(p + d) - g_k(p)``; ``t_k = delta_k / sqrt(0.81 + delta_k^2)``; ``e = (t_0 - t_1)^2``;
      ``s(p) = sum_d e / (0.1 + e)``.
    - Robust term: ``rho(p) = (s(p) + 0.01)^0.4``.
    - ``M(p) = mask(p)`` on interior pixels and 0 elsewhere. ``mask`` is (B, 1, H, W), float or bool. ``None`` means 1.
      In the intended use it is ``~occluded``.
    - ``loss = sum M rho / (sum M + 1e-6)``, summed over the whole batch. The reductions are fp64 in a fixed order.
    - ``return_map=True`` also returns ``s`` as (B, 1, H, W) fp32. It is 0 outside the interior and not differentiable.
    - Gradients go to ``frame0`` and ``frame1``, and only to those that ``needs_input_grad`` asks for. The mask gets
      none.
    - If H or W is smaller than ``patch``, the loss and both gradients are exactly 0. The same holds for an all-zero
      mask.
    - Non-finite frame values make the result unspecified.

    Returns a 0-dim fp32 tensor on the inputs' device with no host synchronisation (or ``(loss, s)``). GPU tensors run
    the native op on the current stream (``torch.ops.oflow.census_loss``): the frames are read once, nothing of the 48
    shifted planes is ever materialised, and both directions are bit-identical from run to run. CPU tensors run the same
    arithmetic as a differentiable torch composition, in fp32 -- or, when a frame is float64, in float64 with a float64
    result, which is what ``torch.autograd.gradcheck`` needs.
    """
    what = "census_loss"
    tensors = (("frame0", frame0), ("frame1", frame1)) + ((("mask", mask),) if mask is not None else ())
    for name, t in tensors:
        if not isinstance(t, Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if not (t.is_floating_point() or (name == "mask" and t.dtype == torch.bool)):
            raise TypeError(f"{what}: {name} must be a floating-point{' or bool' if name == 'mask' else ''} tensor, "
                            f"got {t.dtype}")
    if frame0.dim() != 4 or frame0.shape != frame1.shape:
        raise ValueError(f"{what}: frame0 {tuple(frame0.shape)} and frame1 {tuple(frame1.shape)} must be equal "
                         "(B, C, H, W)")
    b, _, h, w = frame0.shape
    if mask is not None and tuple(mask.shape) != (b, 1, h, w):
        raise ValueError(f"{what}: mask must be (B, 1, H, W) = {(b, 1, h, w)}, got {tuple(mask.shape)}")
    if frame1.device != frame0.device or (mask is not None and mask.device != frame0.device):
        raise ValueError(f"{what}: all tensors must be on one device")
    if isinstance(patch, bool) or not isinstance(patch, int):
        raise TypeError(f"{what}: patch must be an int, got {type(patch).__name__}")
    if patch not in PATCHES:
        raise ValueError(f"{what}: patch must be one of {PATCHES}, got {patch!r}")
    if not 0.0 < float(image_range) < float("inf"):
        raise ValueError(f"{what}: image_range must be a positive finite number, got {image_range!r}")
    if frame0.is_cuda:
        loss, _sum_m, s_map = _native.census_loss(frame0, frame1, None if mask is None else mask.detach(), patch,
                                                  image_range)
    else:
        dtype = torch.float64 if torch.float64 in (frame0.dtype, frame1.dtype) else torch.float32
        loss, s_map = census_loss_torch(frame0.to(dtype), frame1.to(dtype), mask, patch, float(image_range))
    return (loss, s_map.detach()) if return_map else loss


def _pair(d0: Tensor, d1: Tensor, dd: Tensor):
    """(t_0 - t_1, 1 / n_0, 1 / n_1) of one offset, n_k = sqrt(0.81 + delta_k^2), with dd = delta_0 - delta_1. Where the
    two differences have the same sign the ternaries saturate together and ``t_0 - t_1`` would cancel to nothing in
    fp32, so there it is formed as ``(t_0^2 - t_1^2) / (t_0 + t_1)`` with
    ``t_0^2 - t_1^2 = 0.81 (delta_0 - delta_1)(delta_0 + delta_1) / (n_0 n_1)^2``, which is the same number without the
    cancellation; the kernel does the same (csrc/census_loss.hip)."""
    r0, r1 = 1.0 / torch.sqrt(0.81 + d0 * d0), 1.0 / torch.sqrt(0.81 + d1 * d1)
    t0, t1 = d0 * r0, d1 * r1
    same = ((d0 > 0) & (d1 > 0)) | ((d0 < 0) & (d1 < 0))
    rr = r0 * r1
    careful = (0.81 * dd) * (d0 + d1) * (rr * rr) / torch.where(same, t0 + t1, torch.ones_like(t0))
    return torch.where(same, careful, t0 - t1), r0, r1


class _PairTerm(torch.autograd.Function):
    """``e / (0.1 + e)``, ``e = (t_0 - t_1)^2``, of one offset from the two grey differences and their difference
    ``dd`` (a helper: it gets no gradient of its own), with the derivative in the contract's closed form
    (``dt_k / ddelta_k = 0.81 / n_k^3``): autograd's own chain through ``delta / n`` is ``1 / n - delta^2 / n^3``,
    which cancels to nothing in fp32 once ``|delta|`` passes a few dozen grey levels."""

    @staticmethod
    def forward(ctx, d0: Tensor, d1: Tensor, dd: Tensor) -> Tensor:
        ctx.save_for_backward(d0, d1, dd)
        df, _, _ = _pair(d0, d1, dd)
        e = df * df
        return e / (0.1 + e)

    @staticmethod
    def backward(ctx, grad: Tensor):
        d0, d1, dd = ctx.saved_tensors
        df, r0, r1 = _pair(d0, d1, dd)
        q = 0.1 + df * df
        w = grad * ((0.2 * df) / (q * q))
        return w * (0.81 * (r0 * r0 * r0)), -w * (0.81 * (r1 * r1 * r1)), None


def census_loss_torch(frame0: Tensor, frame1: Tensor, mask: Optional[Tensor], patch: int,
                      image_range: float) -> Tuple[Tensor, Tensor]:
    """``census_loss`` as a plain torch composition in the frames' dtype (the CPU path; on a GPU it is the ATen baseline
    the native op is measured against): the contract step by step, one shifted plane pair per offset, the two sums in
    float64. Returns (loss 0-dim in the frames' dtype, s (B, 1, H, W) fp32)."""
    b, c, h, w = frame0.shape
    r = patch // 2
    dtype = frame0.dtype
    if h < patch or w < patch or b == 0 or c == 0:
        zero = (frame0.sum() + frame1.sum()) * 0.0 if frame0.numel() else frame0.new_zeros(())
        return zero, frame0.new_zeros((b, 1, h, w), dtype=torch.float32)
    scale = 255.0 / (image_range * c)

    def channel_sum(f: Tensor) -> Tensor:
        g = f[:, 0].double()
        for k in range(1, c):  # channels in index order, as the kernel adds them
            g = g + f[:, k].double()
        return g

    # the channel sums and their differences are formed in float64 (exact for fp32 frames) and rounded once, after the
    # grey scale: delta_0, delta_1 and delta_0 - delta_1, which would otherwise cancel between two similar frames
    g0, g1 = channel_sum(frame0), channel_sum(frame1)
    c0, c1 = g0[:, r:h - r, r:w - r], g1[:, r:h - r, r:w - r]
    s = torch.zeros_like(c0, dtype=dtype)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy == 0 and dx == 0:
                continue
            d0 = g0[:, r + dy:h - r + dy, r + dx:w - r + dx] - c0
            d1 = g1[:, r + dy:h - r + dy, r + dx:w - r + dx] - c1
            s = s + _PairTerm.apply((d0 * scale).to(dtype), (d1 * scale).to(dtype), ((d0 - d1).detach() * scale).to(dtype))
    rho = (s + 0.01) ** 0.4
    if mask is None:
        m = torch.ones_like(rho)
    else:
        m = mask.detach()[:, 0, r:h - r, r:w - r].to(dtype)
    loss = ((m * rho).double().sum() / (m.double().sum() + 1e-6)).to(dtype)
    s_map = torch.nn.functional.pad(s.detach().float(), (r, r, r, r)).unsqueeze(1)
    return loss, s_map
