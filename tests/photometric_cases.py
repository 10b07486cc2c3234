"""Cases, float64 references and tolerances of the photometric losses (optical_flow.losses.ssim_loss and
charbonnier_loss; include/oflow.h states the contracts). Not a test module: tests/test_photometric_host.py and
tests/test_gpu_photometric.py import it, tools/photometric_bench.py takes the torch compositions from it.

Every case is seeded fp32 input (the frames and masks of tests/losses_cases.py). The references are NumPy float64
restatements of the two contracts in the plain textbook form, written with shifted slices and independent of the package
(the window weights included: normalised in float64, rounded to fp32, and C1, C2, eps, alpha and image_range rounded to
fp32 as the contract says); the closed-form gradients are the plain form's,

    dL/dx(q) = -sum_p g(p) w(q - p) [dSSIM/dmu_x + 2 dSSIM/dv_x (x(q) - mu_x - k mu_x) + dSSIM/dc_xy (y(q) - mu_y - k mu_y)],

k = 1 - (sum w)^2, g(p) = GRAD_LOSS M(p) / (sum M + 1e-6) / (2 C), in scatter form, and ``bound`` is the same closed form
summed over the absolute values of its three terms per element. tests/test_photometric_host.py checks these gradients
against torch autograd in float64 over the plain form (``ssim_plain_torch`` below).

Tolerances. The loss is a sum of non-negative terms on the non-negative frames of every case: |loss - ref| <= K_L * 2^-24
* ref (+ REF_FLOOR for the SSIM reference's own float64 error, below). A gradient element: |g - ref| <= K_G * 2^-24 *
bound + 2^-126. The SSIM map: |map - ref| <= K_M * 2^-24 * (1 + mean_c |1 - SSIM_c|) on the interior, and exactly 0
outside. Every K is calibrated, not chosen: four times what the
torch composition of the operator on fp32 tensors (the package's CPU path) needs against the float64 reference over
the committed cases, rounded up; the factor of four covers the device's division, sqrtf and powf and its summation
order. The measured maxima are in MEASURED, and tests/test_photometric_host.py asserts that the composition stays within
K / 4. A NaN or inf in anything that is checked counts as an infinite error.

What keeps the K's small: 1 - SSIM is formed as (A1 v_d + dm^2 B2) / ((A1 + dm^2) B2) from dm = sum w (x - y) and
v_d = sum w ((x - y) - dm)^2, with x - y formed in float64 and rounded once, and the gradient is derived from that form
(include/oflow.h). With that form alone the composition needed 5.0e3 x 2^-24 of the gradient bound on the "constant"
cases (the means' rounding under a flat window) and 1.1e2 on the uncorrelated "noise" ones at window 11
((e - dm) - csl (x - mu_x) cancels where csl is near 1), so operator and composition also (a) take the window sums over
the values less the centre pixel's and (b) form the contrast term's gradient as cs (x - mu_x) - (y - mu_y), cs from c_xy,
where v_d > B2 / 2. The reference below keeps the plain quotient.

The kernel's tile is 64 x 8 output pixels, the census kernel's, so the shapes are the issue's: 23 x 133 is 3 x 3 tiles
with neither dimension a multiple of the tile, 9 x 65 one pixel past a tile edge both ways, 11 x 75 at window 11 one
interior row that crosses a tile edge in x. The Charbonnier kernels take four pixels per thread and 1024 per workgroup,
with 16-byte accesses when H * W is a multiple of 4: 5 x 64 takes that path, 5 x 65 and 33 x 130 the scalar one, and
24 x 132 (added to the issue's four shapes) takes the 16-byte path with more than one workgroup.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from losses_cases import GRAD_LOSS, TINY, U, _ratio, make_frames, make_mask
from optical_flow.losses import charbonnier_loss_torch, ssim_loss_torch

# ---------------------------------------------------------------------------------------------------- calibration
# maxima of (error / (2^-24 * bound)) of the torch composition on fp32 CPU tensors over the committed cases
MEASURED = {"ssim_loss": 1.842, "ssim_grad": 47.61, "ssim_map": 2.319, "charb_loss": 1.585, "charb_grad": 4.409}
K_SSIM_LOSS = 4 * 2.0   # (2x3x23x133-w11g1.5-constant-one_image)
K_SSIM_GRAD = 4 * 50.0  # (2x3x11x75-w11-noise-none: uncorrelated frames, 121 taps per element)
K_SSIM_MAP = 4 * 2.5    # (2x3x23x133-w11g1.5-noise-none)
K_CHARB_LOSS = 4 * 2.0  # (2x3x5x65-a0.45-noise-none)
K_CHARB_GRAD = 4 * 5.0  # (2x3x33x130-a0.45-near-bool)
# The float64 reference's own error: its plain 1 - SSIM is a difference of numbers near 1, good to a few 2^-53, which
# shows only where the true loss is 0 (identical frames: the reference gives +-1e-17). Allowed on top of the loss bound.
REF_FLOOR = 2.0**-45


def _f32(v: float) -> float:
    return float(np.float32(v))


def window_weights(window: int, sigma: Optional[float]) -> np.ndarray:
    """The contract's 1-D weights: normalised in float64, rounded to fp32 (returned as float64 values)."""
    r = window // 2
    if sigma is None:
        w = [1.0 / window] * window
    else:
        w = [math.exp(-((i - r) ** 2) / (2.0 * sigma**2)) for i in range(window)]
        total = math.fsum(w)
        w = [v / total for v in w]
    return np.asarray(w, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- SSIM cases
class SsimCase(NamedTuple):
    name: str
    frame0: np.ndarray  # (B, C, H, W) fp32
    frame1: np.ndarray
    mask: Optional[np.ndarray]  # (B, 1, H, W) fp32 or bool, or None
    window: int
    sigma: Optional[float]
    image_range: float


FRAME_KINDS = ["noise", "near", "identical", "constant", "range1"]
MASK_KINDS = ["none", "float", "bool", "zero", "one_image"]
SSIM_SHAPES = [((1, 1, 3, 3), 3), ((1, 3, 2, 20), 3), ((1, 3, 9, 70), 11), ((2, 3, 11, 75), 11), ((1, 3, 9, 65), 3),
               ((1, 3, 9, 65), 5), ((1, 2, 40, 9), 7), ((2, 3, 23, 133), 3), ((2, 3, 23, 133), 7), ((2, 3, 23, 133), 11)]


def make_ssim_case(shape, window: int, sigma: Optional[float], frames: str, mask: str) -> SsimCase:
    f0, f1, image_range = make_frames(frames, shape)
    name = "{}x{}x{}x{}-w{}{}-{}-{}".format(*shape, window, "" if sigma is None else f"g{sigma}", frames, mask)
    return SsimCase(name, f0, f1, make_mask(mask, shape), window, sigma, image_range)


def _ssim_cases():
    out = [make_ssim_case(s, w, None, "noise", "none") for s, w in SSIM_SHAPES]
    out += [make_ssim_case(s, w, None, "near", "float") for s, w in SSIM_SHAPES]
    big = (2, 3, 23, 133)
    out += [make_ssim_case(big, 7, None, "near", m) for m in ("none", "bool", "zero", "one_image")]
    out += [make_ssim_case(big, 7, None, k, "none") for k in ("identical", "constant")]
    out += [make_ssim_case(big, 7, None, "range1", "float"), make_ssim_case(big, 3, None, "constant", "bool")]
    # the Gaussian windows: sigma 1.5 at 11 (the standard SSIM window) and 0.8 at 5
    out += [make_ssim_case(big, 11, 1.5, "noise", "none"), make_ssim_case(big, 11, 1.5, "near", "float"),
            make_ssim_case((2, 3, 11, 75), 11, 1.5, "near", "bool"), make_ssim_case(big, 11, 1.5, "identical", "float"),
            make_ssim_case(big, 11, 1.5, "range1", "none"), make_ssim_case(big, 11, 1.5, "constant", "one_image")]
    out += [make_ssim_case((1, 3, 9, 65), 5, 0.8, "noise", "none"), make_ssim_case((1, 3, 9, 65), 5, 0.8, "near", "float"),
            make_ssim_case(big, 5, 0.8, "near", "none"), make_ssim_case(big, 9, None, "near", "float")]
    return out


SSIM_CASES = _ssim_cases()
SSIM_BY_NAME = {c.name: c for c in SSIM_CASES}
SSIM_IDS = [c.name for c in SSIM_CASES]
assert len(SSIM_BY_NAME) == len(SSIM_CASES)


def ssim_constants(case: SsimCase, k1: float = 0.01, k2: float = 0.03) -> Tuple[float, float]:
    return _f32((k1 * case.image_range) ** 2), _f32((k2 * case.image_range) ** 2)


class SsimReference(NamedTuple):
    loss: float
    bound_loss: float  # the same sum over |1 - SSIM_c|
    sum_m: float
    ssim: np.ndarray  # (B, 1, H, W): mean_c SSIM_c, 0 outside the interior
    bound_map: np.ndarray
    grads: Tuple[np.ndarray, np.ndarray]  # dL/dframe_k for dL/dloss = GRAD_LOSS
    bounds: Tuple[np.ndarray, np.ndarray]


@functools.lru_cache(maxsize=None)
def _ssim_reference(name: str) -> SsimReference:
    case = SSIM_BY_NAME[name]
    b, c, h, w = case.frame0.shape
    n, r = case.window, case.window // 2
    ssim_map, bound_map = np.zeros((b, 1, h, w)), np.zeros((b, 1, h, w))
    zeros = lambda: np.zeros((b, c, h, w))  # noqa: E731
    if h < n or w < n:
        return SsimReference(0.0, 0.0, 0.0, ssim_map, bound_map, (zeros(), zeros()), (zeros(), zeros()))
    wt = window_weights(n, case.sigma)
    c1, c2 = ssim_constants(case)
    k = 1.0 - float(wt.sum()) ** 2
    x, y = case.frame0.astype(np.float64), case.frame1.astype(np.float64)
    hi, wi = h - 2 * r, w - 2 * r
    offsets = [(dy, dx) for dy in range(n) for dx in range(n)]
    at = lambda t, dy, dx: t[:, :, dy:dy + hi, dx:dx + wi]  # noqa: E731  (t(p + d), d = (dy - r, dx - r))
    mx = sum(wt[dy] * wt[dx] * at(x, dy, dx) for dy, dx in offsets)
    my = sum(wt[dy] * wt[dx] * at(y, dy, dx) for dy, dx in offsets)
    vx = sum(wt[dy] * wt[dx] * (at(x, dy, dx) - mx) ** 2 for dy, dx in offsets)
    vy = sum(wt[dy] * wt[dx] * (at(y, dy, dx) - my) ** 2 for dy, dx in offsets)
    cxy = sum(wt[dy] * wt[dx] * (at(x, dy, dx) - mx) * (at(y, dy, dx) - my) for dy, dx in offsets)
    s1, s2, t1, t2 = 2 * mx * my + c1, 2 * cxy + c2, mx * mx + my * my + c1, vx + vy + c2
    ssim = s1 * s2 / (t1 * t2)
    d = (0.5 * (1.0 - ssim)).mean(axis=1)
    m = np.ones_like(d) if case.mask is None else case.mask[:, 0, r:h - r, r:w - r].astype(np.float64)
    sum_m = float(m.sum())
    loss = float((m * d).sum() / (sum_m + 1e-6))
    bound_loss = float((m * (0.5 * np.abs(1.0 - ssim)).mean(axis=1)).sum() / (sum_m + 1e-6))
    ssim_map[:, 0, r:h - r, r:w - r] = ssim.mean(axis=1)
    bound_map[:, 0, r:h - r, r:w - r] = 1.0 + np.abs(1.0 - ssim).mean(axis=1)
    # the closed-form gradient in scatter form: pixel p adds to q = p + d
    g = (GRAD_LOSS * m / (sum_m + 1e-6) / (2 * c))[:, None]
    d_mu = (s2 / t2 * 2 * (my * t1 - s1 * mx) / (t1 * t1), s2 / t2 * 2 * (mx * t1 - s1 * my) / (t1 * t1))
    d_v = -s1 * s2 / (t1 * t2 * t2)
    d_c = 2 * s1 / (t1 * t2)
    grads, bounds = (zeros(), zeros()), (zeros(), zeros())
    for dy, dx in offsets:
        wd = wt[dy] * wt[dx]
        a, bb = at(x, dy, dx) - mx, at(y, dy, dx) - my
        for i, (own, other, mu_own, mu_other) in enumerate(((a, bb, mx, my), (bb, a, my, mx))):
            terms = (d_mu[i], 2 * d_v * (own - k * mu_own), d_c * (other - k * mu_other))
            at(grads[i], dy, dx)[...] -= g * wd * sum(terms)
            at(bounds[i], dy, dx)[...] += np.abs(g) * wd * sum(np.abs(t) for t in terms)
    return SsimReference(loss, bound_loss, sum_m, ssim_map, bound_map, grads, bounds)


def ssim_reference(case: SsimCase) -> SsimReference:
    """The float64 reference of a committed case: computed once and shared; callers do not modify it."""
    return _ssim_reference(case.name)


def frame_tensors(case, device="cpu", requires_grad: bool = False, dtype=torch.float32):
    f0, f1 = (torch.from_numpy(f).to(device=device, dtype=dtype).requires_grad_(requires_grad)
              for f in (case.frame0, case.frame1))
    mask = None if case.mask is None else torch.from_numpy(case.mask).to(device)
    return f0, f1, mask


def _np(t) -> np.ndarray:
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def _assert_finite(what: str, name: str, **values) -> None:
    for key, v in values.items():
        if v is not None:
            assert np.isfinite(_np(v)).all(), (what, name, f"{key} has a non-finite element")


def _grad_ratio(grads, ref_grads, ref_bounds) -> float:
    return max([_ratio(np.abs(_np(g) - r), bd, TINY) for g, r, bd in zip(grads, ref_grads, ref_bounds) if g is not None]
               or [0.0])


def ssim_ratios(case: SsimCase, loss=None, grads=None, ssim_map=None) -> dict:
    """error / (2^-24 * bound) of whatever is given: {"loss": .., "grad": .., "map": ..}"""
    ref = ssim_reference(case)
    out = {}
    if loss is not None:
        out["loss"] = _ratio(np.abs(_np(loss) - ref.loss), np.asarray(ref.bound_loss), REF_FLOOR)
    if grads is not None:
        out["grad"] = _grad_ratio(grads, ref.grads, ref.bounds)
    if ssim_map is not None:
        out["map"] = _ratio(np.abs(_np(ssim_map) - ref.ssim), ref.bound_map)
    return out


def assert_ssim(case: SsimCase, what: str, loss=None, grads=None, ssim_map=None, scale: float = 1.0) -> None:
    """``scale``: 1 for the device, 1 / 4 for the composition the K's were calibrated on."""
    g0, g1 = grads if grads is not None else (None, None)
    _assert_finite(what, case.name, loss=loss, grad_frame0=g0, grad_frame1=g1, ssim_map=ssim_map)
    got = ssim_ratios(case, loss, grads, ssim_map)
    print(f"{what} {case.name}: " + ", ".join(f"{k} {v:.3g}" for k, v in got.items()))
    for key, k in (("loss", K_SSIM_LOSS), ("grad", K_SSIM_GRAD), ("map", K_SSIM_MAP)):
        if key in got:
            assert got[key] <= k * scale, (what, case.name, key, got[key], k * scale)
    if ssim_map is not None:
        outside = ssim_reference(case).bound_map == 0
        assert not _np(ssim_map)[outside].any(), (what, case.name, "the map is not 0 outside the interior")


def ssim_compose(frame0, frame1, mask, case: SsimCase):
    """The torch composition of the operator in the frames' dtype, on whatever device they are: (loss, SSIM map)."""
    c1, c2 = ssim_constants(case)
    return ssim_loss_torch(frame0, frame1, mask, window_weights(case.window, case.sigma).tolist(), c1, c2)


def ssim_plain_torch(frame0, frame1, mask, case: SsimCase):
    """The contract's plain textbook form as differentiable torch (float64 tensors): what the reference's closed-form
    gradient is checked against."""
    b, c, h, w = frame0.shape
    n, r = case.window, case.window // 2
    wt = window_weights(n, case.sigma)
    c1, c2 = ssim_constants(case)
    hi, wi = h - 2 * r, w - 2 * r
    offsets = [(dy, dx) for dy in range(n) for dx in range(n)]
    at = lambda t, dy, dx: t[:, :, dy:dy + hi, dx:dx + wi]  # noqa: E731
    mx = sum(wt[dy] * wt[dx] * at(frame0, dy, dx) for dy, dx in offsets)
    my = sum(wt[dy] * wt[dx] * at(frame1, dy, dx) for dy, dx in offsets)
    vx = sum(wt[dy] * wt[dx] * (at(frame0, dy, dx) - mx) ** 2 for dy, dx in offsets)
    vy = sum(wt[dy] * wt[dx] * (at(frame1, dy, dx) - my) ** 2 for dy, dx in offsets)
    cxy = sum(wt[dy] * wt[dx] * (at(frame0, dy, dx) - mx) * (at(frame1, dy, dx) - my) for dy, dx in offsets)
    ssim = (2 * mx * my + c1) * (2 * cxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    d = (0.5 * (1.0 - ssim)).mean(dim=1)
    m = torch.ones_like(d) if mask is None else mask[:, 0, r:h - r, r:w - r].to(d.dtype)
    return (m * d).sum() / (m.sum() + 1e-6)


# ------------------------------------------------------------------------------------------------ Charbonnier cases
class CharbCase(NamedTuple):
    name: str
    frame0: np.ndarray
    frame1: np.ndarray
    mask: Optional[np.ndarray]
    eps: float
    alpha: float
    image_range: float


CHARB_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 64), (2, 3, 5, 65), (2, 3, 33, 130), (2, 3, 24, 132)]
CHARB_PARAMS = [(1e-3, 0.5), (1e-3, 0.45)]


def make_charb_case(shape, eps: float, alpha: float, frames: str, mask: str) -> CharbCase:
    f0, f1, image_range = make_frames(frames, shape)
    name = "{}x{}x{}x{}-a{}-{}-{}".format(*shape, alpha, frames, mask)
    return CharbCase(name, f0, f1, make_mask(mask, shape), eps, alpha, image_range)


def _charb_cases():
    out = []
    for eps, alpha in CHARB_PARAMS:
        out += [make_charb_case(s, eps, alpha, "noise", "none") for s in CHARB_SHAPES]
        out += [make_charb_case(s, eps, alpha, "near", "float") for s in CHARB_SHAPES]
        big = (2, 3, 33, 130)
        out += [make_charb_case(big, eps, alpha, "near", m) for m in ("bool", "zero", "one_image")]
        out += [make_charb_case(big, eps, alpha, k, "none") for k in ("identical", "constant")]
        out += [make_charb_case(big, eps, alpha, "range1", "float"), make_charb_case((2, 3, 24, 132), eps, alpha, "near", "bool")]
    return out


CHARB_CASES = _charb_cases()
CHARB_BY_NAME = {c.name: c for c in CHARB_CASES}
CHARB_IDS = [c.name for c in CHARB_CASES]
assert len(CHARB_BY_NAME) == len(CHARB_CASES)


class CharbReference(NamedTuple):
    loss: float
    sum_m: float
    grads: Tuple[np.ndarray, np.ndarray]
    bounds: Tuple[np.ndarray, np.ndarray]


@functools.lru_cache(maxsize=None)
def _charb_reference(name: str) -> CharbReference:
    case = CHARB_BY_NAME[name]
    b, c, h, w = case.frame0.shape
    eps, alpha, rng = _f32(case.eps), _f32(case.alpha), _f32(case.image_range)
    z = (case.frame0.astype(np.float64) - case.frame1.astype(np.float64)) / rng
    q = z * z + eps * eps
    rho = (q**alpha).mean(axis=1, keepdims=True)
    m = np.ones_like(rho) if case.mask is None else case.mask.astype(np.float64)
    sum_m = float(m.sum())
    loss = float((m * rho).sum() / (sum_m + 1e-6))
    g = GRAD_LOSS * m / (sum_m + 1e-6) * (2 * alpha / (c * rng)) * z * q ** (alpha - 1)
    return CharbReference(loss, sum_m, (g, -g), (np.abs(g), np.abs(g)))


def charb_reference(case: CharbCase) -> CharbReference:
    """The float64 reference of a committed case: computed once and shared; callers do not modify it."""
    return _charb_reference(case.name)


def charb_ratios(case: CharbCase, loss=None, grads=None) -> dict:
    ref = charb_reference(case)
    out = {}
    if loss is not None:
        out["loss"] = _ratio(np.abs(_np(loss) - ref.loss), np.asarray(ref.loss))
    if grads is not None:
        out["grad"] = _grad_ratio(grads, ref.grads, ref.bounds)
    return out


def assert_charb(case: CharbCase, what: str, loss=None, grads=None, scale: float = 1.0) -> None:
    g0, g1 = grads if grads is not None else (None, None)
    _assert_finite(what, case.name, loss=loss, grad_frame0=g0, grad_frame1=g1)
    got = charb_ratios(case, loss, grads)
    print(f"{what} {case.name}: " + ", ".join(f"{k} {v:.3g}" for k, v in got.items()))
    for key, k in (("loss", K_CHARB_LOSS), ("grad", K_CHARB_GRAD)):
        if key in got:
            assert got[key] <= k * scale, (what, case.name, key, got[key], k * scale)


def charb_compose(frame0, frame1, mask, case: CharbCase):
    """The torch composition of the operator in the frames' dtype, on whatever device they are."""
    return charbonnier_loss_torch(frame0, frame1, mask, _f32(case.eps), _f32(case.alpha), _f32(case.image_range))
