"""Cases, float64 references and tolerances of the unsupervised losses (optical_flow.losses; include/oflow.h states the
contracts). Not a test module: tests/test_losses_host.py and tests/test_gpu_losses.py import it, tools/losses_bench.py
takes the torch compositions from it.

Every case is seeded fp32 input. The references are NumPy float64 restatements of the two contracts, written with
shifted slices and independent of the package; the closed-form gradients are the contract's formulas (for the census loss
the scatter form of grad g_k(q) = -sum_d A_k(q, d) + sum_d A_k(q - d, d)), and ``bound`` is the same closed form summed
over the absolute values of its terms per element.

Tolerances. The loss is a sum of non-negative terms: |loss - ref| <= K_L * 2^-24 * ref. A gradient element:
|g - ref| <= K_x * 2^-24 * bound_x + 2^-126. The census map: |s - ref| <= K_S * 2^-24 * bound_s, bound_s the sum over
the offsets of e / (0.1 + e) plus the first-order effect of one rounding of every grey value and of t_0, t_1 on it.
Every K is calibrated, not chosen: four times what the torch composition of the operator on fp32 tensors (the package's
CPU path) needs against the float64 reference over the committed cases, rounded up; the factor of four covers the
device's sqrt, division, powf and expf, its summation order, and the fp32 rounding of what is saved between forward and
backward (the census map). The measured maxima are in MEASURED, and tests/test_losses_host.py asserts that the
composition stays within K / 4. A NaN or inf in anything that is checked counts as an infinite error.

What keeps the K's small. t_0 - t_1 cancels where both ternaries saturate near +-1 -- in fp32 they round to the same
float once |delta| passes ~200 grey levels -- and delta_0 - delta_1 cancels between two similar frames. With the plain
fp32 forms the composition needed 1.7e7 x 2^-24 of bound_x (an error of the whole term) on the "near" cases. Operator
and composition therefore (a) form the channel sums and the three differences delta_0, delta_1, delta_0 - delta_1 in
float64, which is exact for fp32 frames, and round each once, (b) where delta_0 and delta_1 have the same sign, form
t_0 - t_1 as (t_0^2 - t_1^2) / (t_0 + t_1) with t_0^2 - t_1^2 = 0.81 (delta_0 - delta_1)(delta_0 + delta_1) /
(n_0 n_1)^2, and (c) use the contract's closed form 0.81 / n^3 for dt / ddelta, where autograd's own chain
1 / n - delta^2 / n^3 cancels. The smoothness stencil is likewise formed in float64 and rounded once. The float64
reference below keeps the contract's plain forms.
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from optical_flow.losses import census_loss_torch, smoothness_loss_torch

U = 2.0**-24
TINY = 2.0**-126
GRAD_LOSS = 1.75  # dL/dloss of every backward case (exact in fp32)

# ---------------------------------------------------------------------------------------------------- calibration
# maxima of (error / (2^-24 * bound)) of the torch composition on fp32 CPU tensors over the committed cases
MEASURED = {"census_loss": 1.175, "census_grad": 18.42, "census_map": 5.09, "smooth_loss": 3.61, "smooth_grad": 96.6}
K_CENSUS_LOSS = 4 * 1.5   # (1x1x7x7-p7-noise-none: one term, the rounding of powf's result)
K_CENSUS_GRAD = 4 * 20.0  # (2x3x7x70-p7-near-float)
K_CENSUS_MAP = 4 * 5.5    # (2x3x23x133-p7-noise-none: 48 terms added one after another in fp32)
K_SMOOTH_LOSS = 4 * 4.0   # (2x3x33x130-o2-gauss-noise)
K_SMOOTH_GRAD = 4 * 100.0  # (2x3x33x130-o1-gauss-noise: exp arguments near -50, whose rounding exp multiplies by 50)


def _rng(*key) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---------------------------------------------------------------------------------------------------- census cases
class CensusCase(NamedTuple):
    name: str
    frame0: np.ndarray  # (B, C, H, W) fp32
    frame1: np.ndarray
    mask: Optional[np.ndarray]  # (B, 1, H, W) fp32 or bool, or None
    patch: int
    image_range: float


# the kernel's tile is 64 x 8 output pixels: 23 x 133 is 3 x 3 tiles with neither dimension a multiple of the tile,
# 9 x 65 is one pixel past a tile edge both ways, 15 x 71 puts interior pixels into the tile past the edge
CENSUS_SHAPES = [(1, 1, 7, 7), (1, 3, 6, 20), (2, 3, 7, 70), (2, 3, 7, 71), (1, 2, 40, 9), (2, 3, 23, 133), (1, 3, 9, 65),
                 (1, 3, 15, 71)]
FRAME_KINDS = ["noise", "near", "identical", "constant", "range1"]
MASK_KINDS = ["none", "float", "bool", "zero", "one_image"]


def make_frames(kind: str, shape) -> Tuple[np.ndarray, np.ndarray, float]:
    rng = _rng("frames", kind, shape)
    f0 = rng.integers(0, 256, size=shape).astype(np.float32)
    if kind == "noise":
        return f0, rng.integers(0, 256, size=shape).astype(np.float32), 255.0
    if kind == "near":
        return f0, (f0 + rng.normal(0.0, 4.0, size=shape)).astype(np.float32), 255.0
    if kind == "identical":
        return f0, f0.copy(), 255.0
    if kind == "constant":
        return np.full(shape, 37.0, np.float32), np.full(shape, 201.0, np.float32), 255.0
    if kind == "range1":
        a = rng.random(size=shape).astype(np.float32)
        return a, np.clip(a + rng.normal(0.0, 4.0 / 255.0, size=shape), 0.0, 1.0).astype(np.float32), 1.0
    raise ValueError(kind)


def make_mask(kind: str, shape) -> Optional[np.ndarray]:
    b, _, h, w = shape
    rng = _rng("mask", kind, shape)
    if kind == "none":
        return None
    if kind == "float":
        return (rng.random(size=(b, 1, h, w)) < 0.7).astype(np.float32)
    if kind == "bool":
        return rng.random(size=(b, 1, h, w)) < 0.7
    if kind == "zero":
        return np.zeros((b, 1, h, w), np.float32)
    if kind == "one_image":  # the last image of the batch is fully masked
        m = (rng.random(size=(b, 1, h, w)) < 0.7).astype(np.float32)
        m[-1] = 0.0
        return m
    raise ValueError(kind)


def make_census_case(shape, frames: str, mask: str, patch: int = 7) -> CensusCase:
    f0, f1, image_range = make_frames(frames, shape)
    name = "{}x{}x{}x{}-p{}-{}-{}".format(*shape, patch, frames, mask)
    return CensusCase(name, f0, f1, make_mask(mask, shape), patch, image_range)


def _census_cases():
    out = [make_census_case(s, "noise", "none") for s in CENSUS_SHAPES]
    out += [make_census_case(s, "near", "float") for s in CENSUS_SHAPES]
    big = (2, 3, 23, 133)
    out += [make_census_case(big, "near", m) for m in ("none", "bool", "zero", "one_image")]
    out += [make_census_case(big, k, "none") for k in ("identical", "constant")]
    out += [make_census_case(big, "range1", "float"), make_census_case((1, 2, 40, 9), "near", "bool")]
    out += [make_census_case((1, 3, 9, 70), k, "none", patch=p) for p in (3, 5) for k in ("noise", "near")]
    out += [make_census_case((1, 3, 9, 70), "near", "float", patch=p) for p in (3, 5)]
    return out


CENSUS_CASES = _census_cases()
CENSUS_BY_NAME = {c.name: c for c in CENSUS_CASES}
CENSUS_IDS = [c.name for c in CENSUS_CASES]
assert len(CENSUS_BY_NAME) == len(CENSUS_CASES)


class CensusReference(NamedTuple):
    loss: float
    sum_m: float
    s: np.ndarray  # (B, 1, H, W)
    bound_s: np.ndarray
    grads: Tuple[np.ndarray, np.ndarray]  # dL/dframe_k for dL/dloss = GRAD_LOSS
    bounds: Tuple[np.ndarray, np.ndarray]


@functools.lru_cache(maxsize=None)
def _census_reference(name: str) -> CensusReference:
    case = CENSUS_BY_NAME[name]
    b, c, h, w = case.frame0.shape
    p, r = case.patch, case.patch // 2
    scale = 255.0 / (case.image_range * c)
    s_map, bound_s = np.zeros((b, 1, h, w)), np.zeros((b, 1, h, w))
    zeros = lambda: np.zeros((b, c, h, w))  # noqa: E731
    if h < p or w < p:
        return CensusReference(0.0, 0.0, s_map, bound_s, (zeros(), zeros()), (zeros(), zeros()))
    g = [f.astype(np.float64).sum(axis=1) * scale for f in (case.frame0, case.frame1)]
    ctr = (slice(None), slice(r, h - r), slice(r, w - r))
    offsets = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (dy, dx) != (0, 0)]

    def nb(dy, dx):
        return (slice(None), slice(r + dy, h - r + dy), slice(r + dx, w - r + dx))

    def pair(dy, dx):
        d = [gk[nb(dy, dx)] - gk[ctr] for gk in g]
        n = [np.sqrt(0.81 + dk * dk) for dk in d]
        t = [dk / nk for dk, nk in zip(d, n)]
        e = (t[0] - t[1]) ** 2
        dphi = 0.2 * (t[0] - t[1]) / (0.1 + e) ** 2  # d[e / (0.1 + e)] / dt_0 (= -d/dt_1)
        u = [0.81 / nk**3 for nk in n]  # dt_k / ddelta_k
        return t, e, dphi, u

    s = np.zeros_like(g[0][ctr])
    bs = np.zeros_like(s)
    for dy, dx in offsets:
        t, e, dphi, u = pair(dy, dx)
        s += e / (0.1 + e)
        reach = sum(uk * (np.abs(gk[nb(dy, dx)]) + np.abs(gk[ctr])) for uk, gk in zip(u, g))
        bs += e / (0.1 + e) + np.abs(dphi) * (reach + np.abs(t[0]) + np.abs(t[1]))
    rho = (s + 0.01) ** 0.4
    m = np.ones_like(s) if case.mask is None else case.mask[:, 0][ctr].astype(np.float64)
    sum_m = float(m.sum())
    loss = float((m * rho).sum() / (sum_m + 1e-6))
    s_map[:, 0][ctr], bound_s[:, 0][ctr] = s, bs
    cfac = GRAD_LOSS * m / (sum_m + 1e-6) * 0.4 * (s + 0.01) ** -0.6
    gg = [np.zeros_like(g[0]), np.zeros_like(g[0])]
    ga = [np.zeros_like(g[0]), np.zeros_like(g[0])]
    for dy, dx in offsets:
        _, _, dphi, u = pair(dy, dx)
        for k, sign in ((0, 1.0), (1, -1.0)):
            a = cfac * sign * dphi * u[k]  # A_k(p, d)
            gg[k][ctr] -= a
            gg[k][nb(dy, dx)] += a
            ga[k][ctr] += np.abs(a)
            ga[k][nb(dy, dx)] += np.abs(a)
    spread = lambda x: np.broadcast_to((x * scale)[:, None], (b, c, h, w)).copy()  # noqa: E731
    return CensusReference(loss, sum_m, s_map, bound_s, (spread(gg[0]), spread(gg[1])), (spread(ga[0]), spread(ga[1])))


def census_reference(case: CensusCase) -> CensusReference:
    """The float64 reference of a committed case: computed once and shared; callers do not modify it."""
    return _census_reference(case.name)


def census_tensors(case: CensusCase, device="cpu", requires_grad: bool = False, dtype=torch.float32):
    f0, f1 = (torch.from_numpy(f).to(device=device, dtype=dtype).requires_grad_(requires_grad)
              for f in (case.frame0, case.frame1))
    mask = None if case.mask is None else torch.from_numpy(case.mask).to(device)
    return f0, f1, mask


def _np(t) -> np.ndarray:
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def _ratio(err: np.ndarray, bound: np.ndarray, floor: float = 0.0) -> float:
    """max of (err - floor) / (2^-24 * bound); an error where the bound is 0, and a non-finite error (a NaN or inf
    in what is checked), is infinite"""
    err = np.asarray(err, dtype=np.float64)
    if not np.isfinite(err).all():
        return float("inf")
    err = np.maximum(err - floor, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err > 0, err / (U * bound), 0.0)
    return float(np.max(q)) if q.size else 0.0


def _assert_finite(what: str, name: str, **values) -> None:
    for key, v in values.items():
        if v is not None:
            assert np.isfinite(_np(v)).all(), (what, name, f"{key} has a non-finite element")


def census_ratios(case: CensusCase, loss=None, grads=None, s_map=None) -> dict:
    """error / (2^-24 * bound) of whatever is given: {"loss": .., "grad": .., "map": ..}"""
    ref = census_reference(case)
    out = {}
    if loss is not None:
        out["loss"] = _ratio(np.abs(_np(loss) - ref.loss), np.asarray(ref.loss))
    if grads is not None:
        out["grad"] = max([_ratio(np.abs(_np(g) - r), bd, TINY) for g, r, bd in zip(grads, ref.grads, ref.bounds)
                           if g is not None] or [0.0])
    if s_map is not None:
        out["map"] = _ratio(np.abs(_np(s_map) - ref.s), ref.bound_s)
    return out


def assert_census(case: CensusCase, what: str, loss=None, grads=None, s_map=None) -> None:
    g0, g1 = grads if grads is not None else (None, None)
    _assert_finite(what, case.name, loss=loss, grad_frame0=g0, grad_frame1=g1, s_map=s_map)
    got = census_ratios(case, loss, grads, s_map)
    print(f"{what} {case.name}: " + ", ".join(f"{k} {v:.3g}" for k, v in got.items()))
    for key, k in (("loss", K_CENSUS_LOSS), ("grad", K_CENSUS_GRAD), ("map", K_CENSUS_MAP)):
        if key in got:
            assert got[key] <= k, (what, case.name, key, got[key], k)
    if s_map is not None:
        outside = census_reference(case).bound_s == 0
        assert not _np(s_map)[outside].any(), (what, case.name, "s is not 0 outside the interior")


def census_compose(frame0, frame1, mask, patch: int, image_range: float):
    """The torch composition of the operator in the frames' dtype, on whatever device they are: (loss, s map)."""
    return census_loss_torch(frame0, frame1, mask, patch, float(image_range))


# ------------------------------------------------------------------------------------------------ smoothness cases
class SmoothCase(NamedTuple):
    name: str
    flow: np.ndarray  # (B, 2, H, W) fp32
    image: np.ndarray  # (B, C, H, W) fp32
    order: int
    edge_weight: float
    image_range: float


SMOOTH_SHAPES = [(1, 1, 1, 1), (1, 3, 1, 9), (2, 3, 2, 2), (2, 3, 5, 64), (2, 3, 5, 65), (2, 3, 33, 130)]


def make_smooth_case(shape, order: int, flow: str, image: str) -> SmoothCase:
    b, c, h, w = shape
    rng = _rng("smooth", shape, order, flow, image)
    if flow == "gauss":
        fl = rng.normal(0.0, 2.0, size=(b, 2, h, w)).astype(np.float32)
    else:  # a constant flow: every difference is 0
        fl = np.broadcast_to(np.array([1.5, -0.25], np.float32).reshape(1, 2, 1, 1), (b, 2, h, w)).copy()
    image_range = 255.0
    if image == "noise":  # integer levels: almost every edge weight underflows towards 0
        im = rng.integers(0, 256, size=shape).astype(np.float32)
    elif image == "smooth":  # edge weights of order 0.1 .. 1
        im = (100.0 + rng.normal(0.0, 1.5, size=shape)).astype(np.float32)
    elif image == "constant":
        im = np.full(shape, 80.0, np.float32)
    else:  # "range1": frames in [0, 1]
        im = (0.5 + 0.01 * rng.random(size=shape)).astype(np.float32)
        image_range = 1.0
    name = "{}x{}x{}x{}-o{}-{}-{}".format(*shape, order, flow, image)
    return SmoothCase(name, fl, im, order, 150.0, image_range)


def _smooth_cases():
    out = [make_smooth_case(s, o, "gauss", "smooth") for s in SMOOTH_SHAPES for o in (1, 2)]
    big = (2, 3, 33, 130)
    for o in (1, 2):
        out += [make_smooth_case(big, o, "gauss", "noise"), make_smooth_case(big, o, "const", "smooth"),
                make_smooth_case(big, o, "gauss", "range1"), make_smooth_case((2, 3, 5, 65), o, "gauss", "constant")]
    return out


SMOOTH_CASES = _smooth_cases()
SMOOTH_BY_NAME = {c.name: c for c in SMOOTH_CASES}
SMOOTH_IDS = [c.name for c in SMOOTH_CASES]
assert len(SMOOTH_BY_NAME) == len(SMOOTH_CASES)


class SmoothReference(NamedTuple):
    loss: float
    grad: np.ndarray  # dL/dflow for dL/dloss = GRAD_LOSS
    bound: np.ndarray


@functools.lru_cache(maxsize=None)
def _smooth_reference(name: str) -> SmoothReference:
    case = SMOOTH_BY_NAME[name]
    f, im, o = case.flow.astype(np.float64), case.image.astype(np.float64), case.order
    k = float(np.float32(case.edge_weight)) / float(np.float32(case.image_range))
    stencil = (-1.0, 1.0) if o == 1 else (1.0, -2.0, 1.0)
    loss, grad, bound = 0.0, np.zeros_like(f), np.zeros_like(f)
    for axis in (3, 2):
        n = f.shape[axis]
        if n <= o:
            continue  # an empty domain contributes 0

        def cut(t, a, axis=axis, n=n):
            idx = [slice(None)] * 4
            idx[axis] = slice(a, a + n - o)
            return tuple(idx)

        d = sum(cj * f[cut(f, j)] for j, cj in enumerate(stencil))
        wgt = np.exp(-k * np.abs(im[cut(im, o)] - im[cut(im, 0)]).mean(axis=1, keepdims=True))
        psi = np.sqrt(d * d + 1e-6)
        loss += 0.5 * float((wgt * psi).sum()) / d.size
        dl = GRAD_LOSS * 0.5 / d.size * wgt * (d / psi)
        for j, cj in enumerate(stencil):
            grad[cut(f, j)] += cj * dl
            bound[cut(f, j)] += np.abs(cj * dl)
    return SmoothReference(loss, grad, bound)


def smooth_reference(case: SmoothCase) -> SmoothReference:
    """The float64 reference of a committed case: computed once and shared; callers do not modify it."""
    return _smooth_reference(case.name)


def smooth_tensors(case: SmoothCase, device="cpu", requires_grad: bool = False, dtype=torch.float32):
    flow = torch.from_numpy(case.flow).to(device=device, dtype=dtype).requires_grad_(requires_grad)
    return flow, torch.from_numpy(case.image).to(device=device, dtype=dtype)


def smooth_ratios(case: SmoothCase, loss=None, grad=None) -> dict:
    ref = smooth_reference(case)
    out = {}
    if loss is not None:
        out["loss"] = _ratio(np.abs(_np(loss) - ref.loss), np.asarray(ref.loss))
    if grad is not None:
        out["grad"] = _ratio(np.abs(_np(grad) - ref.grad), ref.bound, TINY)
    return out


def assert_smooth(case: SmoothCase, what: str, loss=None, grad=None) -> None:
    _assert_finite(what, case.name, loss=loss, grad_flow=grad)
    got = smooth_ratios(case, loss, grad)
    print(f"{what} {case.name}: " + ", ".join(f"{k} {v:.3g}" for k, v in got.items()))
    for key, k in (("loss", K_SMOOTH_LOSS), ("grad", K_SMOOTH_GRAD)):
        if key in got:
            assert got[key] <= k, (what, case.name, key, got[key], k)


def smooth_compose(flow, image, order: int, edge_weight: float, image_range: float):
    """The torch composition of the operator in the flow's dtype, on whatever device it is."""
    return smoothness_loss_torch(flow, image, order, float(edge_weight), float(image_range))
