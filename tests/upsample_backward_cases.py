"""Float64 closed form, error bounds and deterministic inputs of the convex-upsampling backward tests
(csrc/upsample_backward.hip). PyTorch on the CPU only; inputs come from seeded ``torch.Generator``s, so every machine
rebuilds them bit for bit. Not a test module.

Notation (csrc/upsample.hip's header): F_k(c, y, x) = 8 * flow[n, c, y + k/3 - 1, x + k%3 - 1] (zero outside the
grid), w_k(i, j, y, x) = softmax_k(mask[n, k*64 + i*8 + j, y, x]), g_c = grad_out[n, c, 8y + i, 8x + j],
a_k = sum_c g_c F_k(c). Then
    grad_mask[n, k*64 + i*8 + j, y, x] = w_k (a_k - sum_k' w_k' a_k')
    S_k(c, y, x)                       = sum_{i, j} w_k g_c
    grad_flow[n, c, y', x']            = 8 sum_k S_k(c, y' - (k/3 - 1), x' - (k%3 - 1))    (source pixel inside the grid)
"""
from __future__ import annotations

from typing import List, NamedTuple, Tuple

import torch
import torch.nn.functional as F

# (B, H, W): centre tap only; a single row; a single column; exactly one 32-px segment; one pixel past a segment; two
# segments plus one pixel; one pixel short of a segment
SHAPES = [(1, 1, 1), (2, 1, 9), (1, 9, 1), (2, 5, 32), (3, 7, 33), (1, 2, 65), (2, 9, 31)]
MASK_SIGMAS = [0.0, 3.0, 30.0]  # uniform weights, ordinary, saturated softmax
FLOW_SIGMA = 6.0

U = 2.0**-24  # fp32 unit roundoff
# Tolerance constants: four times what the reference's own fp32 ATen composition needs on the CPU over CASES below
# (tests/test_upsample_backward_host.py::test_reference_fp32_autograd_calibrates_the_tolerance measures it and asserts
# it stays within K / 4); the factor of four is for the device's expf and summation order, which differ from the CPU's.
# Measured maxima over the committed cases: grad_flow 7.79 U * bound_flow (the single-sub-pixel case: one term, so the
# relative error of its small softmax weight is not averaged away; the Gaussian cases need 1.45), grad_mask
# 35.32 U * bound_mask * (1 + d) (the saturated 2x9x31 case). Rounded up to 8.0 and 35.5, so that the host check does
# not hinge on the last digit of one CPU's summation order, then times four.
K_F = 32.0
K_M = 142.0
UNDERFLOW = 1e-30  # times 8 max|flow| max|grad_out|: a saturated weight that underflows in fp32


class Case(NamedTuple):
    name: str
    grad_out: torch.Tensor  # (B, 2, 8H, 8W) fp32
    flow: torch.Tensor  # (B, 2, H, W) fp32
    mask: torch.Tensor  # (B, 576, H, W) fp32


def gaussian(seed: int, shape, sigma: float = 1.0) -> torch.Tensor:
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * sigma


def make_case(shape: Tuple[int, int, int], sigma: float, single: bool = False) -> Case:
    b, h, w = shape
    seed = 100000 * b + 1000 * h + 10 * w + int(sigma)
    flow = gaussian(seed + 1, (b, 2, h, w), FLOW_SIGMA)
    mask = gaussian(seed + 2, (b, 576, h, w), sigma)
    g = gaussian(seed + 3, (b, 2, 8 * h, 8 * w))
    name = f"{b}x{h}x{w}-s{sigma:g}"
    if single:  # zero except in one sub-pixel (i, j) = (5, 3) of the low-res pixel (h // 2, w // 2) of the last image
        one = torch.zeros_like(g)
        yy, xx = 8 * (h // 2) + 5, 8 * (w // 2) + 3
        one[b - 1, :, yy, xx] = g[b - 1, :, yy, xx]
        g, name = one, name + "-single"
    return Case(name, g, flow, mask)


CASES: List[Case] = [make_case(sh, s) for sh in SHAPES for s in MASK_SIGMAS] + [make_case((3, 7, 33), 3.0, single=True)]
CASE_IDS = [c.name for c in CASES]


def _parts(grad_out: torch.Tensor, flow: torch.Tensor, mask: torch.Tensor, absolute: bool):
    n, _, h, w = flow.shape
    g = grad_out.double().reshape(n, 2, h, 8, w, 8).permute(0, 1, 3, 5, 2, 4)  # (n, c, i, j, y, x)
    fp = F.pad(8.0 * flow.double(), (1, 1, 1, 1))
    taps = torch.stack([fp[:, :, k // 3 : k // 3 + h, k % 3 : k % 3 + w] for k in range(9)], dim=2)  # F_k: (n, c, k, y, x)
    wts = torch.softmax(mask.double().reshape(n, 9, 8, 8, h, w), dim=1)  # (n, k, i, j, y, x)
    if absolute:
        g, taps = g.abs(), taps.abs()
    a = torch.einsum("ncijyx,nckyx->nkijyx", g, taps)
    return g, wts, a


def _gather(s: torch.Tensor) -> torch.Tensor:
    """grad_flow from S (n, c, k, y, x): 8 * sum_k S_k(c, y' - (k/3 - 1), x' - (k%3 - 1)), zero outside the grid."""
    h, w = s.shape[-2:]
    sp = F.pad(s, (1, 1, 1, 1))
    return 8.0 * sum(sp[:, :, k, 2 - k // 3 : 2 - k // 3 + h, 2 - k % 3 : 2 - k % 3 + w] for k in range(9))


def backward64(grad_out: torch.Tensor, flow: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(grad_flow (B, 2, H, W), grad_mask (B, 576, H, W)) in float64 by the closed form above."""
    g, wts, a = _parts(grad_out, flow, mask, False)
    gm = wts * (a - (wts * a).sum(dim=1, keepdim=True))
    s = torch.einsum("nkijyx,ncijyx->nckyx", wts, g)
    return _gather(s), gm.reshape(mask.shape)


def bounds64(grad_out: torch.Tensor, flow: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The same form on absolute values: bound_flow = 8 sum_k sum_ij w_k |g_c| at the source pixels, bound_mask =
    w_k (|a|_k + sum_k' w_k' |a|_k') with |a|_k = sum_c |g_c| |F_k(c)|: the operand magnitudes the fp32 rounding error
    of each gradient scales with."""
    g, wts, a = _parts(grad_out, flow, mask, True)
    bm = wts * (a + (wts * a).sum(dim=1, keepdim=True))
    s = torch.einsum("nkijyx,ncijyx->nckyx", wts, g)
    return _gather(s), bm.reshape(mask.shape)


def logit_gap(mask: torch.Tensor) -> torch.Tensor:
    """d = max_k' m_k' - m_k per mask element (B, 576, H, W), float64: the magnitude of the exponent's argument."""
    n, _, h, w = mask.shape
    m = mask.double().reshape(n, 9, 64, h, w)
    return (m.amax(dim=1, keepdim=True) - m).reshape(mask.shape)


def tolerances(case: Case, k_f: float = K_F, k_m: float = K_M) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-element (tol_flow, tol_mask): K_f U bound_flow, and K_m U bound_mask (1 + d) + 1e-30 * 8 max|flow| max|g|
    (the (1 + d) factor: the rounding of the exponent's argument m_k - max; the floor: fp32 underflow of a saturated
    weight)."""
    bf, bm = bounds64(case.grad_out, case.flow, case.mask)
    floor = UNDERFLOW * 8.0 * float(case.flow.abs().max()) * float(case.grad_out.abs().max())
    return k_f * U * bf, k_m * U * bm * (1.0 + logit_gap(case.mask)) + floor


def error_ratios(got_flow, got_mask, case: Case) -> Tuple[float, float]:
    """Worst error in units of U * bound (flow) and U * bound * (1 + d) (mask, after the underflow floor): what K has to
    cover. Elements whose bound is 0 must be exact (flow) / within the floor (mask)."""
    rf, rm = backward64(case.grad_out, case.flow, case.mask)
    tf, tm = tolerances(case, 1.0, 1.0)
    floor = UNDERFLOW * 8.0 * float(case.flow.abs().max()) * float(case.grad_out.abs().max())
    ef = (got_flow.double() - rf).abs()
    em = ((got_mask.double() - rm).abs() - floor).clamp(min=0.0)
    assert bool((ef[tf == 0] == 0).all()) and bool((em[tm <= floor] == 0).all()), case.name
    live_f, live_m = tf > 0, tm > floor
    kf = float((ef[live_f] / tf[live_f]).max()) if bool(live_f.any()) else 0.0
    km = float((em[live_m] / (tm[live_m] - floor)).max()) if bool(live_m.any()) else 0.0
    return kf, km


_REFERENCES = {}


def reference(case: Case):
    """(grad_flow, grad_mask, tol_flow, tol_mask) of a committed case in float64, computed once per process."""
    if case.name not in _REFERENCES:
        _REFERENCES[case.name] = backward64(case.grad_out, case.flow, case.mask) + tolerances(case)
    return _REFERENCES[case.name]


def assert_close(got_flow, got_mask, case: Case, what: str) -> None:
    """Each given gradient (None: not checked) within its tolerance of float64, element by element."""
    rf, rm, tf, tm = reference(case)
    for name, got, ref, tol in (("grad_flow", got_flow, rf, tf), ("grad_mask", got_mask, rm, tm)):
        if got is None:
            continue
        assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float32, (what, case.name, name, got.shape)
        got = got.detach().cpu().double()
        assert bool(torch.isfinite(got).all()), (what, case.name, name, "not finite")
        err = (got - ref).abs()
        worst = float((err / tol.clamp(min=1e-300)).max())
        print(f"{what} {case.name} {name}: max |err| = {float(err.max()):.3e}, worst err / tol = {worst:.3f}")
        assert bool((err <= tol).all()), (what, case.name, name, worst)
