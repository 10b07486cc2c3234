"""``ssim_loss`` and ``charbonnier_loss``: the SSIM and robust L1 photometric terms (include/oflow.h
``oflow_ssim_loss_f32`` and ``oflow_charbonnier_loss_f32`` state the contracts)."""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from .. import _native

WINDOWS = (3, 5, 7, 9, 11)


def _f32(v: float) -> float:
    """``v`` rounded to fp32, as a Python float: the value the C ABI receives."""
    return torch.tensor(float(v), dtype=torch.float32).item()


def ssim_window(window: int, sigma: Optional[float]) -> List[float]:
    """The 1-D weights of the separable SSIM window: a box (``sigma=None``) or a Gaussian, normalised in float64 and
    rounded to fp32. The fp32 values are the contract's weights (they add up to 1 only to rounding)."""
    r = window // 2
    if sigma is None:
        w = [1.0 / window] * window
    else:
        w = [math.exp(-((i - r) ** 2) / (2.0 * float(sigma) ** 2)) for i in range(window)]
        total = math.fsum(w)
        w = [v / total for v in w]
    return torch.tensor(w, dtype=torch.float64).float().tolist()


def _check_frames(what: str, frame0, frame1, mask, image_range) -> None:
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
    if not 0.0 < float(image_range) < float("inf"):
        raise ValueError(f"{what}: image_range must be a positive finite number, got {image_range!r}")


def ssim_loss(
    frame0: Tensor,
    frame1: Tensor,
    mask: Optional[Tensor] = None,
    window: int = 3,
    sigma: Optional[float] = None,
    image_range: float = 255.0,
    k1: float = 0.01,
    k2: float = 0.03,
    return_map: bool = False,
):
    """The SSIM loss between two frames under a ``window`` x ``window`` box or Gaussian window (an addition; the
    reference has none): the structural photometric term of UnFlow, UFlow and ARFlow, and -- with ``window=11,
    sigma=1.5, return_map=True`` -- the standard SSIM map for scoring a warped or interpolated frame.

    ``frame0`` and ``frame1`` are (B, C, H, W). In a training loss ``frame1`` is the second image already warped back.

    - ``window`` is one of {3, 5, 7, 9, 11}, ``r = window // 2``. The window is separable, ``w(dy, dx) = w[dy] w[dx]``:
      a box (``w[i] = 1 / window``) when ``sigma`` is None, else a Gaussian (``w[i]`` proportional to
      ``exp(-(i - r)^2 / (2 sigma^2))``). The weights are normalised in float64 and rounded to fp32; the fp32 values are
      the contract's weights.
    - The frames are used as they are (no division of the input): ``C1 = (k1 image_range)^2``,
      ``C2 = (k2 image_range)^2``, each rounded to fp32.
    - Interior pixels are those with ``r <= y < H - r`` and ``r <= x < W - r`` (a "valid" filter, as ``census_loss``).
    - For an interior pixel p and channel c, with sums over the window: ``mu_x = sum w x``, ``mu_y`` likewise;
      ``v_x = sum w (x - mu_x)^2``, ``v_y`` likewise; ``c_xy = sum w (x - mu_x)(y - mu_y)``;
      ``SSIM_c = (2 mu_x mu_y + C1)(2 c_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(v_x + v_y + C2))``.
    - ``d(p) = mean_c (1 - SSIM_c) / 2``, not clamped: with C1, C2 > 0 it lies in [0, 1] already.
    - ``M(p) = mask(p)`` on interior pixels and 0 elsewhere. ``mask`` is (B, 1, H, W), float or bool. ``None`` means 1.
    - ``loss = sum M d / (sum M + 1e-6)``, summed over the whole batch. The reductions are fp64 in a fixed order.
    - ``return_map=True`` also returns ``mean_c SSIM_c`` as (B, 1, H, W) fp32. It is 0 outside the interior, detached
      and not differentiable.
    - Gradients go to ``frame0`` and ``frame1``, and only to those that ``needs_input_grad`` asks for. The mask gets
      none.
    - If H or W is smaller than ``window``, the loss and both gradients are exactly 0. The same holds for an all-zero
      mask. On identical non-negative frames the loss is exactly 0.
    - Non-finite frame values make the result unspecified.

    ``1 - SSIM`` is not taken from the quotient above, which loses everything on the near-identical frames a good flow
    produces: with ``A1 = 2 mu_x mu_y + C1``, ``B2 = v_x + v_y + C2``, ``dm = sum w (x - y)`` and
    ``v_d = sum w ((x - y) - dm)^2`` it is ``(A1 v_d + dm^2 B2) / ((A1 + dm^2) B2)``, the differences ``x - y`` formed
    in float64 and rounded once; the gradient is derived from that form too (include/oflow.h).

    Returns a 0-dim fp32 tensor on the inputs' device with no host synchronisation (or ``(loss, map)``). GPU tensors run
    the native op on the current stream (``torch.ops.oflow.ssim_loss``): each frame is read once plus the halo, none of
    the filtered planes is materialised, and both directions are bit-identical from run to run. CPU tensors run the same
    arithmetic as a differentiable torch composition, in fp32 -- or, when a frame is float64, in float64 with a float64
    result, which is what ``torch.autograd.gradcheck`` needs.
    """
    what = "ssim_loss"
    _check_frames(what, frame0, frame1, mask, image_range)
    if isinstance(window, bool) or not isinstance(window, int):
        raise TypeError(f"{what}: window must be an int, got {type(window).__name__}")
    if window not in WINDOWS:
        raise ValueError(f"{what}: window must be one of {WINDOWS}, got {window!r}")
    if sigma is not None and not 0.0 < float(sigma) < float("inf"):
        raise ValueError(f"{what}: sigma must be None (a box) or a positive finite number, got {sigma!r}")
    for name, k in (("k1", k1), ("k2", k2)):
        if not 0.0 < float(k) < float("inf"):
            raise ValueError(f"{what}: {name} must be a positive finite number, got {k!r}")
    weights = ssim_window(window, sigma)
    c1, c2 = _f32((float(k1) * float(image_range)) ** 2), _f32((float(k2) * float(image_range)) ** 2)
    if not (c1 > 0.0 and c2 > 0.0 and math.isfinite(c1) and math.isfinite(c2)):
        raise ValueError(f"{what}: (k1 image_range)^2 and (k2 image_range)^2 must be positive finite fp32 numbers")
    if frame0.is_cuda:
        loss, _sum_m, ssim_map = _native.ssim_loss(frame0, frame1, None if mask is None else mask.detach(), weights, c1,
                                                   c2, return_map)
    else:
        dtype = torch.float64 if torch.float64 in (frame0.dtype, frame1.dtype) else torch.float32
        loss, ssim_map = ssim_loss_torch(frame0.to(dtype), frame1.to(dtype), mask, weights, c1, c2)
    return (loss, ssim_map.detach()) if return_map else loss


def _shifted(t: Tensor, dy: int, dx: int, hi: int, wi: int) -> Tensor:
    """t(p + d) for every interior pixel p, d = (dy - r, dx - r)"""
    return t[..., dy:dy + hi, dx:dx + wi]


def _offset_of_mean(t: Tensor, weights: List[float], k: float) -> Tuple[Tensor, Tensor]:
    """(t(p), mu(p) - t(p)) on the interior, mu = sum_d w(d) t(p + d): the window sum is taken over the values less the
    centre pixel's, row by row (columns first) as the kernel adds it, so a flat neighbourhood keeps its small
    deviations. ``k = 1 - (sum w)^2``: the fp32 weights do not add up to exactly 1."""
    n = len(weights)
    r = n // 2
    hi, wi = t.shape[-2] - 2 * r, t.shape[-1] - 2 * r
    centre = _shifted(t, r, r, hi, wi)
    out = torch.zeros_like(centre)
    for dy in range(n):
        row = torch.zeros_like(centre)
        for dx in range(n):
            row = row + weights[dx] * (_shifted(t, dy, dx, hi, wi) - centre)
        out = out + weights[dy] * row
    return centre, out - k * centre


def _centred_sum(t: Tensor, centre: Tensor, offset: Tensor, weights: List[float], other=None) -> Tensor:
    """sum_d w(d) (t(p + d) - mu(p))^2 on the interior with t(p + d) - mu(p) = (t(p + d) - t(p)) - offset(p); with
    ``other = (u, its centre, its offset)`` the cross sum sum_d w(d) (t(p + d) - mu_t(p)) (u(p + d) - mu_u(p))."""
    n = len(weights)
    hi, wi = centre.shape[-2:]
    out = torch.zeros_like(centre)
    for dy in range(n):
        row = torch.zeros_like(centre)
        for dx in range(n):
            a = (_shifted(t, dy, dx, hi, wi) - centre) - offset
            b = a if other is None else (_shifted(other[0], dy, dx, hi, wi) - other[1]) - other[2]
            row = row + weights[dx] * (a * b)
        out = out + weights[dy] * row
    return out


class _SsimTerm(torch.autograd.Function):
    """``sum_c (1 - SSIM_c)`` on the interior, (B, C, H, W) x 2 -> (B, H - 2r, W - 2r), in the cancellation-free form,
    with the contract's closed-form gradient (include/oflow.h): the kernel's arithmetic, step by step."""

    @staticmethod
    def forward(ctx, x: Tensor, y: Tensor, weights: List[float], c1: float, c2: float) -> Tensor:
        k = 1.0 - math.fsum(weights) ** 2
        e = (x.double() - y.double()).to(x.dtype)  # exact for fp32 frames, rounded once
        (xp, ox), (yp, oy), (ep, oe) = (_offset_of_mean(t, weights, k) for t in (x, y, e))
        mx, my, dm = xp + ox, yp + oy, ep + oe
        vx, vy, vd = (_centred_sum(t, tp, o, weights) for t, tp, o in ((x, xp, ox), (y, yp, oy), (e, ep, oe)))
        cxy = _centred_sum(x, xp, ox, weights, (y, yp, oy)) if any(ctx.needs_input_grad[:2]) else vd
        ctx.save_for_backward(x, y, e, mx, my, dm, vx, vy, vd, ox, oy, oe, cxy)
        ctx.args = (weights, c1, c2, k)
        a1, b2, dm2 = 2.0 * mx * my + c1, vx + vy + c2, dm * dm
        return ((a1 * vd + dm2 * b2) / ((a1 + dm2) * b2)).sum(dim=1)

    @staticmethod
    def backward(ctx, grad: Tensor):
        x, y, e, mx, my, dm, vx, vy, vd, ox, oy, oe, cxy = ctx.saved_tensors
        weights, c1, c2, k = ctx.args
        a1, b2, dm2 = 2.0 * mx * my + c1, vx + vy + c2, dm * dm
        tt = a1 + dm2
        # cs = (2 c_xy + C2) / B2 = 1 - v_d / B2: whichever of the two is not a difference of near-equal numbers
        far = vd > 0.5 * b2
        cs = torch.where(far, (2.0 * cxy + c2) / b2, 1.0 - vd / b2)
        csl = torch.where(far, 1.0 - cs, vd / b2)
        g = 2.0 * (a1 / tt) / b2
        sum_mu = mx + my
        lum = (2.0 * cs * dm) / (tt * tt)
        fx, fy = lum * (my * sum_mu + c1), -lum * (mx * sum_mu + c1)
        # dF(p)/dx(q) = w (Fx' + al (x(q) - mu_x) + be (y(q) - mu_y) + ga (e(q) - dm)): similar frames (v_d small) take
        # G ((e - dm) - csl (x - mu_x)), dissimilar ones G (cs (x - mu_x) - (y - mu_y)); y with the roles swapped, -ga
        zero = torch.zeros_like(g)
        al, be, ga = torch.where(far, g * cs, -(g * csl)), torch.where(far, -g, zero), torch.where(far, zero, g)
        gm = grad.unsqueeze(1)
        px = gm * ((fx - k * g * (dm - csl * mx)) - (al * ox + be * oy + ga * oe))
        py = gm * ((fy + k * g * (dm + csl * my)) - (al * oy + be * ox - ga * oe))
        al, be, ga = gm * al, gm * be, gm * ga
        n = len(weights)
        r = n // 2
        hi, wi = mx.shape[-2:]
        xp, yp, ep = (_shifted(t, r, r, hi, wi) for t in (x, y, e))
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gx = torch.zeros_like(x) if need_x else None
        gy = torch.zeros_like(y) if need_y else None
        # pixel p adds w(d) (P(p) + al(p) (t(q) - t(p)) + be(p) (u(q) - u(p)) +- ga(p) (e(q) - e(p))) to q = p + d; a row
        # of pixels at a time, columns first, which is the order the kernel's gather adds them in
        w = x.shape[-1]
        for dy in range(n):
            rx = px.new_zeros(px.shape[:-1] + (w,)) if need_x else None
            ry = px.new_zeros(px.shape[:-1] + (w,)) if need_y else None
            for dx in range(n):
                tx, ty = _shifted(x, dy, dx, hi, wi) - xp, _shifted(y, dy, dx, hi, wi) - yp
                ge = ga * (_shifted(e, dy, dx, hi, wi) - ep)
                if need_x:
                    rx[..., dx:dx + wi] += weights[dx] * ((px + ge) + (al * tx + be * ty))
                if need_y:
                    ry[..., dx:dx + wi] += weights[dx] * ((py - ge) + (al * ty + be * tx))
            if need_x:
                gx[..., dy:dy + hi, :] += weights[dy] * rx
            if need_y:
                gy[..., dy:dy + hi, :] += weights[dy] * ry
        return gx, gy, None, None, None


def ssim_loss_torch(frame0: Tensor, frame1: Tensor, mask: Optional[Tensor], weights: List[float], c1: float,
                    c2: float) -> Tuple[Tensor, Tensor]:
    """``ssim_loss`` as a torch composition in the frames' dtype (the CPU path; on a GPU it is the baseline the native op
    is measured against): the contract step by step in the kernel's arithmetic, the two sums in float64. ``weights``: the
    1-D window (``ssim_window``). Returns (loss 0-dim in the frames' dtype, mean_c SSIM (B, 1, H, W) fp32)."""
    b, c, h, w = frame0.shape
    n = len(weights)
    r = n // 2
    dtype = frame0.dtype
    if h < n or w < n or b == 0 or c == 0:
        zero = (frame0.sum() + frame1.sum()) * 0.0 if frame0.numel() else frame0.new_zeros(())
        return zero, frame0.new_zeros((b, 1, h, w), dtype=torch.float32)
    fsum = _SsimTerm.apply(frame0, frame1, weights, c1, c2)
    d = fsum * (0.5 / c)
    if mask is None:
        m = torch.ones_like(d)
    else:
        m = mask.detach()[:, 0, r:h - r, r:w - r].to(dtype)
    loss = ((m * d).double().sum() / (m.double().sum() + 1e-6)).to(dtype)
    ssim_map = torch.nn.functional.pad((1.0 - fsum.detach() / c).float(), (r, r, r, r)).unsqueeze(1)
    return loss, ssim_map


def charbonnier_loss(
    frame0: Tensor,
    frame1: Tensor,
    mask: Optional[Tensor] = None,
    eps: float = 1e-3,
    alpha: float = 0.5,
    image_range: float = 255.0,
):
    """The Charbonnier (robust L1) loss between two frames (an addition; the reference has none): the generalised
    photometric term of UnFlow / UFlow / ARFlow, ``alpha = 0.5`` the classic one and ``0.45`` the common robust choice.

    ``frame0`` and ``frame1`` are (B, C, H, W). In a training loss ``frame1`` is the second image already warped back.

    - ``rho(p) = mean_c (((x - y) / image_range)^2 + eps^2)^alpha`` on every pixel (there is no interior).
    - ``loss = sum M rho / (sum M + 1e-6)`` with ``M = mask``, (B, 1, H, W), float or bool; ``None`` means 1. The
      reductions are fp64 in a fixed order.
    - ``x - y`` is formed in float64 (exact for fp32 frames) and rounded once. ``eps``, ``alpha`` and ``image_range`` are
      rounded to fp32.
    - ``eps > 0`` and ``0 < alpha <= 1``.
    - The gradient is the closed form ``M / (sum M + 1e-6) * 2 alpha / (C image_range) * z * (z^2 + eps^2)^(alpha - 1)``,
      ``z = (x - y) / image_range``, to ``frame0`` and its negative to ``frame1``, only where ``needs_input_grad``
      asks. The mask gets none. With an all-zero mask the loss and both gradients are exactly 0.
    - Non-finite frame values make the result unspecified.

    Returns a 0-dim fp32 tensor on the inputs' device with no host synchronisation. GPU tensors run the native op on the
    current stream (``torch.ops.oflow.charbonnier_loss``), bit-identical from run to run in both directions. CPU tensors
    run the same arithmetic as a differentiable torch composition, in fp32 -- or in float64 when a frame is float64.
    """
    what = "charbonnier_loss"
    _check_frames(what, frame0, frame1, mask, image_range)
    if not 0.0 < float(eps) < float("inf"):
        raise ValueError(f"{what}: eps must be a positive finite number, got {eps!r}")
    if not 0.0 < float(alpha) <= 1.0:
        raise ValueError(f"{what}: alpha must be in (0, 1], got {alpha!r}")
    eps, alpha, image_range = _f32(eps), _f32(alpha), _f32(image_range)
    if not (eps > 0.0 and alpha > 0.0 and 0.0 < image_range < float("inf")):
        raise ValueError(f"{what}: eps, alpha and image_range must be positive finite fp32 numbers")
    if frame0.is_cuda:
        loss, _sum_m = _native.charbonnier_loss(frame0, frame1, None if mask is None else mask.detach(), eps, alpha,
                                                image_range)
        return loss
    dtype = torch.float64 if torch.float64 in (frame0.dtype, frame1.dtype) else torch.float32
    return charbonnier_loss_torch(frame0.to(dtype), frame1.to(dtype), mask, eps, alpha, image_range)


def charbonnier_loss_torch(frame0: Tensor, frame1: Tensor, mask: Optional[Tensor], eps: float, alpha: float,
                           image_range: float) -> Tensor:
    """``charbonnier_loss`` as a plain torch composition in the frames' dtype (the CPU path; on a GPU it is the ATen
    baseline the native op is measured against). Returns the 0-dim loss in the frames' dtype."""
    b, c, h, w = frame0.shape
    dtype = frame0.dtype
    if frame0.numel() == 0:
        return frame0.new_zeros(())
    z = (frame0.double() - frame1.double()).to(dtype) / image_range  # the difference exact, rounded once
    q = z * z + eps * eps
    p = torch.sqrt(q) if alpha == 0.5 else q ** alpha
    rho = p.sum(dim=1, keepdim=True) * (1.0 / c)
    m = torch.ones_like(rho) if mask is None else mask.detach().to(dtype)
    return ((m * rho).double().sum() / (m.double().sum() + 1e-6)).to(dtype)
