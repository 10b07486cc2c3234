"""Float64 reference, error bounds and deterministic inputs of the forward-warping tests (optical_flow.splat,
csrc/splat.hip, csrc/splat_backward.hip). NumPy / PyTorch on the CPU only, seeded, so every machine rebuilds the inputs
bit for bit. Not a test module.

The contract (include/oflow.h, oflow_splat_f32). Source s = (i, j) of image b lands at px = fp32(j + u), py = fp32(i + v);
it is skipped unless px > -1, px < W, py > -1, py < H. x0 = floor(px), fx = px - x0 (in float64: exact), the four taps
(x0 + dx, y0 + dy) get w = ax[dx] ay[dy], ax = (1 - fx, fx), in float64; taps outside the frame are dropped. With the
per-source weight m (1; the metric; or exp(d), d = fp32(metric - max of the image's metric)),
    N_c(t) = sum w m frame_c(s),   D(t) = sum w m,   out = N ("sum") or N / (D + EPS), EPS = 1e-7.
The reference evaluates exactly this in float64 at the fp32-rounded positions (and, for "soft", at the fp32-rounded d).

Forward error bound, per target pixel t and channel c. The device turns each contribution into an integer multiple of
the quantum q_N = 2^(eN - K) (q_D = 2^(eD - K) for D), K = 62 - ceil(log2(4 H W)), eN / eD the image's exponents:
    dN = n_t q_N / 2                      n_t contributions, each rounded to the nearest quantum
       + (n_t + 8) 2^-53 A_N              forming each product in float64 (three roundings), the int64 -> float64
                                          conversion of the sum, and this reference's own float64 summation;
                                          A_N = sum w m |frame_c|
       + e_m A_N + 2^-126 sum w |frame_c| "soft" only: the device expf's documented error of 1 ulp, e_m = 2^-23, on m,
                                          and an absolute 2^-126 where m underflows the normal fp32 range
    dD = the same with frame_c = 1 (A_D = D: every m in the cases is >= 0)
    "sum":   |out - ref| <= dN + 2^-24 |ref| + 2^-149                       (the final rounding to fp32)
    others:  |out - ref| <= (dN + |ref| dD) / (D + EPS - dD) + (2^-24 + 4 2^-53) |ref| + 2^-149
             (the exact perturbation of a quotient; the float64 division and the final rounding)
    weight:  |weight - D| <= dD + 2^-24 D + 2^-149
A pixel that nothing reaches (n_t = 0) must be exactly 0 in both outputs. Nothing here is tuned: emulate() repeats the
fixed-point scheme in NumPy and tests/test_splat_host.py asserts that it stays within this bound on every case.

Backward tolerance (after tests/upsample_backward_cases.py): K_x 2^-24 bound_x + 2^-126 (1 + unit_x) per element, where
bound_x is the closed form of the gradient (closed_form(), the formulas of include/oflow.h) taken over the absolute
values of its terms, unit_x the same with m = 1 (the fp32 underflow of m or of a product with m), and K_x is four times
what an fp32 torch composition of the operator itself needs against float64 autograd on the committed cases (the
factor of four is for the device's expf, its summation order and the fp32 rounding of the saved out and D).
tests/test_splat_host.py::test_fp32_composition_calibrates_the_backward_tolerance measures it and asserts it stays
within K / 4. Measured maxima over the committed cases: MEASURED below.
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

EPS = 1e-7
U24 = 2.0**-24
U53 = 2.0**-53
EXPF_REL = 2.0**-23  # 1 ulp: the documented maximum error of the device's expf
TINY32 = 2.0**-126  # the smallest normal fp32
MODES = {"sum": 0, "avg": 1, "linear": 2, "soft": 3}

# (B, C, H, W): one pixel; a single row; a single column; a quarter wave of pixels per row; one past it; odd sizes under
# one block; several blocks per image with a row length that is no multiple of the wave
SHAPES = [(1, 1, 1, 1), (2, 1, 1, 9), (1, 2, 9, 1), (2, 3, 5, 64), (3, 3, 7, 65), (1, 5, 17, 33), (2, 8, 33, 130)]
FLOW_KINDS = ["zero", "shift", "half", "gauss2", "gaussbig", "collapse", "border", "nonfinite"]
SHIFT = (2, -1)  # the integer shift (dx, dy)
BORDER_TINY = 2.0**-20
# the non-finite entries of the "nonfinite" flow: (value, channel, flat pixel index modulo H * W), in every image
NONFINITE = [(float("nan"), 0, 0), (float("inf"), 1, 7), (float("-inf"), 0, 14), (1e30, 1, 21), (-1e30, 0, 28)]

# what the fp32 composition needed (worst err / (2^-24 bound) over CASES), and the constants: the measured value
# rounded up, times four
MEASURED = {"frame": 16.87, "flow": 5.24, "metric": 10.83}  # (frame and metric: 1x5x17x33-collapse-linear, 561 terms
K_FRAME = 4 * 17.0                                            # added one after another in fp32)
K_FLOW = 4 * 5.5
K_METRIC = 4 * 11.0


class Case(NamedTuple):
    name: str
    mode: str
    frame: np.ndarray  # (B, C, H, W) fp32
    flow: np.ndarray  # (B, 2, H, W) fp32
    metric: Optional[np.ndarray]  # (B, 1, H, W) fp32 or None
    grad_out: np.ndarray  # (B, C, H, W) fp32


def _rng(*key: int) -> np.random.Generator:
    return np.random.default_rng(list(key))


def make_flow(kind: str, shape: Tuple[int, int, int, int]) -> np.ndarray:
    b, _, h, w = shape
    seed = FLOW_KINDS.index(kind)
    flow = np.zeros((b, 2, h, w), np.float32)
    if kind == "shift":
        flow[:, 0], flow[:, 1] = SHIFT
    elif kind == "half":
        flow[:] = 0.5
    elif kind in ("gauss2", "nonfinite"):
        flow = (_rng(1, seed, b, h, w).standard_normal((b, 2, h, w)) * 2.0).astype(np.float32)
        if kind == "nonfinite":
            for value, ch, k in NONFINITE:
                flow.reshape(b, 2, h * w)[:, ch, k % (h * w)] = value
    elif kind == "gaussbig":
        flow = (_rng(1, seed, b, h, w).standard_normal((b, 2, h, w)) * max(h, w)).astype(np.float32)
    elif kind == "collapse":  # every source lands on the centre pixel: H * W contributions to one address
        flow[:, 0] = (w // 2) - np.arange(w, dtype=np.float32)[None, None, :]
        flow[:, 1] = (h // 2) - np.arange(h, dtype=np.float32)[None, :, None]
    elif kind == "border":  # landings at -1 + tiny, exactly W - 1 and W - 1 + 0.5, in x along row 0 and in y along column 0
        for k, (tx, ty) in enumerate(((-1 + BORDER_TINY, -1 + BORDER_TINY), (w - 1.0, h - 1.0), (w - 0.5, h - 0.5))):
            flow[:, 0, 0, k % w] = np.float32(tx) - np.float32(k % w)
            flow[:, 1, k % h, 0] = np.float32(ty) - np.float32(k % h)
    return flow


def make_case(shape, kind: str, mode: str, sigma: float = 2.0, scales=None, tag: str = "") -> Case:
    b, c, h, w = shape
    key = (b, c, h, w, FLOW_KINDS.index(kind), MODES[mode], int(sigma))
    frame = _rng(2, *key).standard_normal(shape).astype(np.float32)
    if scales is not None:
        frame *= np.asarray(scales, np.float32).reshape(b, 1, 1, 1)
    metric = None
    if mode == "soft":
        metric = (_rng(3, *key).standard_normal((b, 1, h, w)) * sigma).astype(np.float32)
    elif mode == "linear":  # exact zeros, so that D can be 0 where sources did land
        r = _rng(3, *key)
        metric = np.abs(r.standard_normal((b, 1, h, w))).astype(np.float32)
        metric[r.random((b, 1, h, w)) < 0.3] = 0.0
    grad_out = _rng(4, *key).standard_normal(shape).astype(np.float32)
    name = f"{b}x{c}x{h}x{w}-{kind}-{mode}" + (f"-s{sigma:g}" if mode == "soft" else "") + tag
    return Case(name, mode, frame, make_flow(kind, shape), metric, grad_out)


def _cases() -> List[Case]:
    out = []
    for shape in SHAPES:
        for kind in FLOW_KINDS:
            out += [make_case(shape, kind, mode) for mode in ("sum", "avg", "linear", "soft")]
        for kind in ("gauss2", "collapse"):  # uniform weights; a saturated softmax whose small weights underflow
            out += [make_case(shape, kind, "soft", sigma) for sigma in (0.0, 30.0)]
    return out


CASES: List[Case] = _cases()
# batch independence: two images whose scales differ by 1e8
MIXED: List[Case] = [make_case((2, 3, 9, 33), "gauss2", mode, scales=(1e4, 1e-4), tag="-mixed") for mode in MODES]
ALL_CASES = CASES + MIXED
BY_NAME: Dict[str, Case] = {c.name: c for c in ALL_CASES}
CASE_IDS = [c.name for c in ALL_CASES]


def frac_bits(h: int, w: int) -> int:
    """K = 62 - ceil(log2(4 H W)) (oflow_splat_frac_bits)."""
    return 62 - (4 * h * w - 1).bit_length()


def _exponent(x: float) -> int:
    return 0 if x == 0 else int(math.frexp(x)[1])


class Geometry(NamedTuple):
    keep: np.ndarray  # (B, HW) bool
    taps: list  # four (ok (B, HW) bool, idx (B, HW) int64 target pixel (0 where not ok), w (B, HW) f64, sx, sy (B, HW) f64)


def geometry(flow: np.ndarray) -> Geometry:
    b, _, h, w = flow.shape
    with np.errstate(invalid="ignore", over="ignore"):
        px = np.arange(w, dtype=np.float32)[None, None, :] + flow[:, 0]  # fp32 sums
        py = np.arange(h, dtype=np.float32)[None, :, None] + flow[:, 1]
        assert px.dtype == np.float32 and py.dtype == np.float32
        keep = (px > -1) & (px < w) & (py > -1) & (py < h)
    pxs, pys = np.where(keep, px, np.float32(0)), np.where(keep, py, np.float32(0))
    x0f, y0f = np.floor(pxs), np.floor(pys)
    fx, fy = pxs.astype(np.float64) - x0f, pys.astype(np.float64) - y0f  # exact in float64 (not always in fp32)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    ax, ay = (1.0 - fx, fx), (1.0 - fy, fy)
    taps = []
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            ok = keep & (x >= 0) & (x < w) & (y >= 0) & (y < h)
            idx = np.where(ok, y * w + x, 0)
            sx = (1.0 if dx else -1.0) * ay[dy]  # dw/dpx
            sy = (1.0 if dy else -1.0) * ax[dx]  # dw/dpy
            taps.append(tuple(a.reshape(b, h * w) for a in (ok, idx, ax[dx] * ay[dy], sx, sy)))
    return Geometry(keep.reshape(b, h * w), taps)


def soft_argument(metric: np.ndarray) -> np.ndarray:
    """d = fp32(metric - max of the image's metric), (B, HW) fp32."""
    b = metric.shape[0]
    m = metric.reshape(b, -1)
    return (m - m.max(axis=1, keepdims=True)).astype(np.float32)


def source_weight(case: Case, device_like: bool = False) -> np.ndarray:
    """m (B, HW) float64; device_like: "soft" rounded to fp32, as the device holds it (correctly rounded here: NumPy's
    own fp32 exp is documented to err by more than the 1 ulp the bound grants the device's expf)."""
    b, _, h, w = case.frame.shape
    if case.mode == "linear":
        return case.metric.reshape(b, h * w).astype(np.float64)
    if case.mode == "soft":
        d = soft_argument(case.metric)
        m = np.exp(d.astype(np.float64))
        return m.astype(np.float32).astype(np.float64) if device_like else m
    return np.ones((b, h * w), np.float64)


def exponents(case: Case) -> Tuple[np.ndarray, np.ndarray]:
    """(eN, eD) per image."""
    b = case.frame.shape[0]
    e_f = [_exponent(float(np.abs(case.frame[i]).max())) for i in range(b)]
    e_m = [_exponent(float(np.abs(case.metric[i]).max())) if case.mode == "linear" else 1 for i in range(b)]
    return np.array([f + m for f, m in zip(e_f, e_m)]), np.array(e_m)


class Reference(NamedTuple):
    out: np.ndarray  # (B, C, H, W) f64
    weight: np.ndarray  # (B, 1, H, W) f64 (D)
    out_bound: np.ndarray
    weight_bound: np.ndarray
    hole: np.ndarray  # (B, 1, H, W) bool: nothing reaches the pixel
    num: np.ndarray  # (B, C, HW) f64 N
    num_abs: np.ndarray  # (B, C, HW) f64 A_N


def _scatter(dst: np.ndarray, ok: np.ndarray, idx: np.ndarray, vals: np.ndarray) -> None:
    """dst (B, HW) += vals (B, HW) at idx where ok."""
    bi = np.broadcast_to(np.arange(dst.shape[0])[:, None], ok.shape)
    np.add.at(dst, (bi[ok], idx[ok]), vals[ok])


_REFERENCES: Dict[str, Reference] = {}


def reference(case: Case) -> Reference:
    """The float64 reference of a case with its per-pixel bounds, computed once per process."""
    if case.name in _REFERENCES:
        return _REFERENCES[case.name]
    b, c, h, w = case.frame.shape
    hw = h * w
    geo = geometry(case.flow)
    m = source_weight(case)
    f = case.frame.reshape(b, c, hw).astype(np.float64)
    num, num_abs, wf = (np.zeros((b, c, hw)) for _ in range(3))
    den, wsum, n = (np.zeros((b, hw)) for _ in range(3))
    for ok, idx, wt, _, _ in geo.taps:
        wm = wt * m
        _scatter(den, ok, idx, wm)
        _scatter(wsum, ok, idx, wt)
        _scatter(n, ok, idx, np.ones_like(wt))
        for ch in range(c):
            _scatter(num[:, ch], ok, idx, wm * f[:, ch])
            _scatter(num_abs[:, ch], ok, idx, np.abs(wm * f[:, ch]))
            _scatter(wf[:, ch], ok, idx, wt * np.abs(f[:, ch]))
    assert (m >= 0).all()  # (so that A_D = D)
    k = frac_bits(h, w)
    e_n, e_d = exponents(case)
    q_n = np.ldexp(1.0, e_n - k).reshape(b, 1, 1)
    q_d = np.ldexp(1.0, e_d - k).reshape(b, 1)
    soft = case.mode == "soft"
    e_m, floor = (EXPF_REL, TINY32) if soft else (0.0, 0.0)
    d_n = n[:, None] * q_n / 2 + (n[:, None] + 8) * U53 * num_abs + e_m * num_abs + floor * wf
    d_d = n * q_d / 2 + (n + 8) * U53 * den + e_m * den + floor * wsum
    if case.mode == "sum":
        out = num
        out_bound = d_n + U24 * np.abs(out) + 2.0**-149
    else:
        out = num / (den[:, None] + EPS)
        room = den + EPS - d_d
        assert (room > 0).all()
        out_bound = (d_n + np.abs(out) * d_d[:, None]) / room[:, None] + (U24 + 4 * U53) * np.abs(out) + 2.0**-149
    weight_bound = d_d + U24 * den + 2.0**-149
    ref = Reference(out.reshape(b, c, h, w), den.reshape(b, 1, h, w), out_bound.reshape(b, c, h, w),
                    weight_bound.reshape(b, 1, h, w), (n == 0).reshape(b, 1, h, w), num, num_abs)
    _REFERENCES[case.name] = ref
    return ref


def emulate(case: Case) -> Tuple[np.ndarray, np.ndarray]:
    """The device's fixed-point scheme in NumPy: (out, weight) fp32. int64 sums of rint(contribution * 2^(K - e)),
    contributions formed as ((w m) frame) in float64, m through an fp32 exp for "soft"."""
    b, c, h, w = case.frame.shape
    hw = h * w
    geo = geometry(case.flow)
    m = source_weight(case, device_like=True)
    f = case.frame.reshape(b, c, hw).astype(np.float64)
    k = frac_bits(h, w)
    e_n, e_d = exponents(case)
    s_n, s_d = np.ldexp(1.0, k - e_n).reshape(b, 1), np.ldexp(1.0, k - e_d).reshape(b, 1)
    num = np.zeros((b, c, hw), np.int64)
    den = np.zeros((b, hw), np.int64)
    for ok, idx, wt, _, _ in geo.taps:
        wm = wt * m
        _scatter(den, ok, idx, np.rint(wm * s_d).astype(np.int64))
        for ch in range(c):
            _scatter(num[:, ch], ok, idx, np.rint((wm * f[:, ch]) * s_n).astype(np.int64))
    assert np.abs(num).max(initial=0) < 2**62 and np.abs(den).max(initial=0) < 2**62
    n64 = num.astype(np.float64) * np.ldexp(1.0, e_n - k).reshape(b, 1, 1)
    d64 = den.astype(np.float64) * np.ldexp(1.0, e_d - k).reshape(b, 1)
    out = n64 if case.mode == "sum" else n64 / (d64[:, None] + EPS)
    return out.astype(np.float32).reshape(b, c, h, w), d64.astype(np.float32).reshape(b, 1, h, w)


def forward_ratios(case: Case, out, weight) -> Tuple[float, float]:
    """Worst |error| / bound of out and of weight; asserts shapes, dtypes and that holes are exactly 0."""
    ref = reference(case)
    out, weight = np.asarray(out), np.asarray(weight)
    assert out.dtype == np.float32 and weight.dtype == np.float32, (case.name, out.dtype, weight.dtype)
    assert out.shape == ref.out.shape and weight.shape == ref.weight.shape, (case.name, out.shape, weight.shape)
    assert np.isfinite(out).all() and np.isfinite(weight).all(), (case.name, "not finite")
    assert not weight[ref.hole].any(), (case.name, "a hole with weight != 0")
    assert not out[np.broadcast_to(ref.hole, out.shape)].any(), (case.name, "a hole with out != 0")
    r_out = np.abs(out.astype(np.float64) - ref.out) / ref.out_bound
    r_w = np.abs(weight.astype(np.float64) - ref.weight) / ref.weight_bound
    return float(r_out.max()), float(r_w.max())


def assert_forward(case: Case, out, weight, what: str) -> None:
    r_out, r_w = forward_ratios(case, out, weight)
    print(f"{what} {case.name}: worst |out - ref| / bound = {r_out:.3f}, |weight - D| / bound = {r_w:.3f}")
    assert r_out <= 1.0 and r_w <= 1.0, (what, case.name, r_out, r_w)


# ------------------------------------------------------------------------------------------------------ backward
def tensors(case: Case, device="cpu", requires_grad: bool = True, dtype=torch.float32):
    """(frame, flow, metric or None) as fresh leaf tensors holding the case's fp32 values."""
    def leaf(a):
        return None if a is None else torch.from_numpy(a.copy()).to(device=device, dtype=dtype).requires_grad_(requires_grad)
    return leaf(case.frame), leaf(case.flow), leaf(case.metric)


def _rounded_fp32(value32: torch.Tensor, leaf: torch.Tensor, dtype) -> torch.Tensor:
    """``value32`` (computed in fp32 from the detached leaf) as a ``dtype`` tensor whose gradient flows to ``leaf`` with
    derivative 1: the contract's fp32-rounded quantities under float64 autograd."""
    leaf = leaf.to(dtype)
    return value32.to(dtype) + (leaf - leaf.detach())


def compose(frame: torch.Tensor, flow: torch.Tensor, metric: Optional[torch.Tensor], mode: str, dtype) -> torch.Tensor:
    """The operator as a differentiable torch composition on CPU leaves that hold fp32 values: the landing positions and
    the soft argument are the contract's fp32-rounded ones, everything after them is ``dtype`` arithmetic; the soft
    shift is detached. Returns out (B, C, H, W) in dtype."""
    b, c, h, w = frame.shape
    hw = h * w
    flow32 = flow.detach().float()
    px = _rounded_fp32(torch.arange(w, dtype=torch.float32).view(1, 1, w) + flow32[:, 0], flow[:, 0], dtype)
    py = _rounded_fp32(torch.arange(h, dtype=torch.float32).view(1, h, 1) + flow32[:, 1], flow[:, 1], dtype)
    keep = (px > -1) & (px < w) & (py > -1) & (py < h)
    pxs, pys = torch.where(keep, px, 0.0), torch.where(keep, py, 0.0)
    x0f, y0f = torch.floor(pxs.detach()), torch.floor(pys.detach())
    fx, fy = pxs - x0f, pys - y0f
    x0, y0 = x0f.long(), y0f.long()
    if mode == "linear":
        m = metric[:, 0].to(dtype)
    elif mode == "soft":
        m32 = metric.detach().float()[:, 0]
        m = torch.exp(_rounded_fp32(m32 - m32.reshape(b, -1).amax(dim=1).view(b, 1, 1), metric[:, 0], dtype))
    else:
        m = torch.ones((b, h, w), dtype=dtype)
    f = frame.to(dtype).permute(1, 0, 2, 3).reshape(c, b * hw)
    num = torch.zeros((c, b * hw), dtype=dtype)
    den = torch.zeros(b * hw, dtype=dtype)
    base = (torch.arange(b) * hw).view(b, 1, 1)
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = x0 + dx, y0 + dy
            ok = keep & (x >= 0) & (x < w) & (y >= 0) & (y < h)
            wm = ((fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy)) * m
            wm = torch.where(ok, wm, torch.zeros_like(wm)).reshape(-1)
            idx = (torch.where(ok, y * w + x, torch.zeros_like(x)) + base).reshape(-1)
            den = den.index_add(0, idx, wm)
            num = num.index_add(1, idx, wm * f)
    out = num if mode == "sum" else num / (den + EPS)
    return out.view(c, b, h, w).permute(1, 0, 2, 3)


def autograd_gradients(case: Case, dtype) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """(grad_frame, grad_flow, grad_metric) of sum(out * grad_out) by autograd through compose(), as float64."""
    frame, flow, metric = tensors(case, dtype=dtype)
    out = compose(frame, flow, metric, case.mode, dtype)
    loss = (out * torch.from_numpy(case.grad_out).to(dtype)).sum()
    leaves = [frame, flow] + ([metric] if metric is not None else [])
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(leaf) if g is None else g for g, leaf in zip(grads, leaves)]
    return grads[0].double(), grads[1].double(), (grads[2].double() if metric is not None else None)


def closed_form(case: Case, absolute: bool = False, unit_m: bool = False):
    """The gradients by the formulas of include/oflow.h in float64 NumPy: (grad_frame (B, C, H, W), grad_flow
    (B, 2, H, W), grad_metric (B, 1, H, W) or None). ``absolute``: every term by its absolute value (the magnitudes the
    rounding errors scale with); ``unit_m``: the final factor m left out (absolute only: the underflow floor)."""
    b, c, h, w = case.frame.shape
    hw = h * w
    ref = reference(case)
    geo = geometry(case.flow)
    m = source_weight(case)
    f = case.frame.reshape(b, c, hw).astype(np.float64)
    g = case.grad_out.reshape(b, c, hw).astype(np.float64)
    den = ref.weight.reshape(b, hw)
    norm = case.mode != "sum"
    r = 1.0 / (den + EPS) if norm else np.ones((b, hw))
    if absolute:
        f, g = np.abs(f), np.abs(g)
        out = ref.num_abs / (den[:, None] + EPS)
        gd = r * (g * out).sum(axis=1) if norm else np.zeros((b, hw))
    else:
        out = ref.out.reshape(b, c, hw)
        gd = -r * (g * out).sum(axis=1) if norm else np.zeros((b, hw))
    big_g = np.zeros((b, c, hw))
    gm = np.zeros((b, hw))
    gx, gy = np.zeros((b, hw)), np.zeros((b, hw))
    for ok, idx, wt, sx, sy in geo.taps:
        wt = np.where(ok, wt, 0.0)
        r_t = np.where(ok, np.take_along_axis(r, idx, axis=1), 0.0)
        gd_t = np.where(ok, np.take_along_axis(gd, idx, axis=1), 0.0)
        rg = r_t[:, None] * np.take_along_axis(g, np.broadcast_to(idx[:, None], (b, c, hw)), axis=2)
        rg = np.where(ok[:, None], rg, 0.0)
        big_g += wt[:, None] * rg
        gm += wt * gd_t
        q = (f * rg).sum(axis=1) + gd_t
        if absolute:
            sx, sy = np.abs(sx), np.abs(sy)
        gx += np.where(ok, sx * q, 0.0)
        gy += np.where(ok, sy * q, 0.0)
    gm = gm + (f * big_g).sum(axis=1)
    mm = np.ones_like(m) if unit_m else (np.abs(m) if absolute else m)
    g_frame = (mm[:, None] * big_g).reshape(b, c, h, w)
    g_flow = np.stack([mm * gx, mm * gy], axis=1).reshape(b, 2, h, w)
    g_metric = None
    if case.mode == "linear":
        g_metric = gm.reshape(b, 1, h, w)
    elif case.mode == "soft":
        g_metric = (mm * gm).reshape(b, 1, h, w)
    return g_frame, g_flow, g_metric


_BACKWARD: Dict[str, tuple] = {}
GRAD_NAMES = ("frame", "flow", "metric")


def backward_reference(case: Case):
    """((ref, bound, floor) per gradient in GRAD_NAMES order; None for a metric gradient that does not exist): float64
    autograd values, the absolute closed form and the underflow floor 2^-126 (1 + unit), computed once per process."""
    if case.name not in _BACKWARD:
        refs = autograd_gradients(case, torch.float64)
        bounds = closed_form(case, absolute=True)
        units = closed_form(case, absolute=True, unit_m=True)
        _BACKWARD[case.name] = tuple(
            None if r is None else (r.numpy(), bd, TINY32 * (1.0 + un)) for r, bd, un in zip(refs, bounds, units))
    return _BACKWARD[case.name]


def backward_ratios(case: Case, grads) -> List[Optional[float]]:
    """Per gradient (None: not given / does not exist) the worst (|err| - floor) / (2^-24 bound): what K has to cover.
    An element whose bound is 0 must be within the floor."""
    out = []
    for got, ref in zip(grads, backward_reference(case)):
        if got is None or ref is None:
            out.append(None)
            continue
        r, bound, floor = ref
        got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
        assert got.shape == r.shape, (case.name, got.shape, r.shape)
        assert np.isfinite(got).all(), (case.name, "not finite")
        err = np.maximum(np.abs(got - r) - floor, 0.0)
        assert not err[bound == 0].any(), (case.name, "an element with a zero bound is off")
        live = bound > 0
        out.append(float((err[live] / (U24 * bound[live])).max()) if live.any() else 0.0)
    return out


def assert_backward(case: Case, grads, what: str) -> None:
    ratios = backward_ratios(case, grads)
    print(f"{what} {case.name}: worst err / (2^-24 bound): " +
          ", ".join(f"{n} {r:.2f}" for n, r in zip(GRAD_NAMES, ratios) if r is not None))
    for name, ratio, k in zip(GRAD_NAMES, ratios, (K_FRAME, K_FLOW, K_METRIC)):
        assert ratio is None or ratio <= k, (what, case.name, name, ratio, k)
