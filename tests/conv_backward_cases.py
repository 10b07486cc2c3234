"""Float64 closed form, error bounds and deterministic inputs of the convolution backward tests
(csrc/conv_backward.hip). PyTorch on the CPU only; inputs come from seeded ``torch.Generator``s, so every machine
rebuilds them bit for bit. Not a test module.

Stride 1, zero padding (kh // 2, kw // 2), odd kh, kw. With oy = ky - kh // 2, ox = kx - kw // 2 and out-of-image terms
zero:
    dx[b, c, y, x]   = sum_{ky, kx, n} gy[b, n, y - oy, x - ox] * w[n, c, ky, kx]     n_x = kh * kw * Cout terms
    dw[n, c, ky, kx] = sum_{b, y, x}   gy[b, n, y, x] * x[b, c, y + oy, x + ox]       n_w = B * H * W terms
    db[n]            = sum_{b, y, x}   gy[b, n, y, x]                                  n_b = B * H * W terms
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

U = 2.0**-24  # fp32 unit roundoff
# The kernels' tiling (csrc/conv_backward.hip: kCT, kWK, kSlab), which the shapes below are chosen around;
# tests/test_conv_backward_host.py checks SLAB against the library's oflow_conv2d_backward_weight_slab_pixels().
PIXEL_TILE = 64  # dgrad: flattened pixels per workgroup tile (and channels per tile, both kernels)
K_CHUNK = 32  # wgrad: pixels per K chunk
SLAB = 2048  # wgrad: flattened pixels per K slab

# Tolerance per element: min(K, n + 2) * U * bound, bound = the element's sum on absolute values, n its number of
# terms. (n + 2) * U * bound is the worst case of an fp32 sum of n products in any order and needs no measurement; K
# keeps the long sums honest (with n = 3500 one misplaced term would slip under the cap alone). K is four times what
# ATen's own fp32 CPU autograd of F.conv2d needs on CASES below
# (tests/test_conv_backward_host.py::test_reference_fp32_autograd_calibrates_the_tolerance measures it and asserts it
# stays within K / 4); the factor of four is for the device's summation order (k-ordered fma chains per tile, slabs
# added in ascending order), which differs from the CPU's.
# Measured maxima over the committed cases, in units of U * bound: dx 4.28 (3x3-c8-n8-3x41x37), dw 4.32 and db 1.80
# (1x5-c384-n128-2x6x40). Rounded up to 5.5, so that the host check does not hinge on one CPU's summation order (the
# thread count and the vector width change ATen's), then times four.
K = 22.0


class Case(NamedTuple):
    name: str
    grad_out: torch.Tensor  # (B, Cout, H, W) fp32
    x: torch.Tensor  # (B, Cin, H, W) fp32
    weight: torch.Tensor  # (Cout, Cin, kh, kw) fp32

    @property
    def dims(self) -> Tuple[int, int, int, int, int, int, int]:
        """(B, Cout, Cin, H, W, kh, kw): the C ABI's argument order."""
        b, cin, h, w = self.x.shape
        cout, _, kh, kw = self.weight.shape
        return b, cout, cin, h, w, kh, kw


def gaussian(seed: int, shape, sigma: float = 1.0) -> torch.Tensor:
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * sigma


# (kh, kw, Cin, Cout, B, H, W)
SHAPES = [
    (1, 1, 2, 2, 1, 1, 1),  # a single product per element
    (3, 3, 33, 2, 2, 1, 1),  # 1x1 image: every tap but the centre leaves it
    (1, 5, 33, 33, 1, 1, 70),  # one row, taps leave on the left and right; channels one past the 32-lane tile
    (5, 1, 2, 126, 1, 70, 1),  # one column, taps leave above and below
    (7, 7, 2, 33, 2, 5, 9),  # convf1's kernel on an image smaller than it: taps leave on every side
    (7, 7, 2, 2, 1, 9, 10),  # and on one it fits into
    (3, 3, 126, 2, 3, 3, 7),  # 63 pixels: one below the pixel tile, three images in it (the flow head's 256 -> 2)
    (3, 3, 33, 126, 2, 4, 8),  # 64 pixels: exactly one tile over two images
    (1, 5, 126, 33, 5, 1, 13),  # 65 pixels: one past the tile, five images
    (5, 1, 33, 33, 2, 7, 6),  # the vertical GRU pass on an image wider than one column
    (1, 1, 324, 33, 2, 3, 5),  # convc1's input width: six channel tiles, the last with 4 channels
    (1, 1, 33, 576, 1, 4, 9),  # the mask head's output width: nine channel tiles
    (1, 5, 8, 8, 3, 1, 11),  # 33 pixels: one past the wgrad K chunk
    (3, 3, 8, 8, 2, 32, 32),  # wgrad K-split: exactly one slab (2048 pixels)
    (1, 5, 8, 8, 3, 1, 683),  # 2049 pixels: a second slab of one pixel
    (3, 3, 8, 8, 3, 41, 37),  # 4551 pixels: two full slabs and a remainder of 455, the slab edges inside images
    (1, 5, 384, 128, 2, 6, 40),  # a real layer at reduced extent: the GRU's horizontal pass
]
GRAD_SIGMA = 1e-3  # the gradient of a mean-reduced loss: far below fp16's normal range after a few layers
WEIGHT_SIGMA = 0.1


def make_case(shape, single: bool = False) -> Case:
    kh, kw, cin, cout, b, h, w = shape
    seed = 1000003 * (kh * 8 + kw) + 10007 * cin + 101 * cout + 1009 * b + 37 * h + w
    x = gaussian(seed + 1, (b, cin, h, w))
    wt = gaussian(seed + 2, (cout, cin, kh, kw), WEIGHT_SIGMA)
    g = gaussian(seed + 3, (b, cout, h, w), GRAD_SIGMA)
    name = f"{kh}x{kw}-c{cin}-n{cout}-{b}x{h}x{w}"
    if single:  # zero except at pixel (h // 2, w // 2) of the last image: most input gradients are exactly 0
        one = torch.zeros_like(g)
        one[b - 1, :, h // 2, w // 2] = g[b - 1, :, h // 2, w // 2]
        g, name = one, name + "-single"
    return Case(name, g, x, wt)


CASES: List[Case] = [make_case(sh) for sh in SHAPES] + [make_case((3, 3, 33, 33, 2, 5, 6), single=True)]
CASE_IDS = [c.name for c in CASES]
BY_NAME: Dict[str, Case] = dict(zip(CASE_IDS, CASES))


def slabs(case: Case) -> int:
    b, _, h, w = case.x.shape
    return (b * h * w + SLAB - 1) // SLAB


def term_counts(case: Case) -> Tuple[int, int, int]:
    """(n_x, n_w, n_b): the number of terms of one element's sum."""
    b, cout, _, h, w, kh, kw = case.dims
    return kh * kw * cout, b * h * w, b * h * w


def _sums(grad_out: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, absolute: bool):
    g, xs, wt = grad_out.double(), x.double(), weight.double()
    if absolute:
        g, xs, wt = g.abs(), xs.abs(), wt.abs()
    h, w = xs.shape[-2:]
    kh, kw = wt.shape[-2:]
    py, px = kh // 2, kw // 2
    gp, xp = F.pad(g, (px, px, py, py)), F.pad(xs, (px, px, py, py))
    dx, dw = torch.zeros_like(xs), torch.zeros_like(wt)
    for ky in range(kh):
        for kx in range(kw):
            oy, ox = ky - py, kx - px
            g_shift = gp[:, :, py - oy : py - oy + h, px - ox : px - ox + w]  # gy[b, n, y - oy, x - ox]
            dx += torch.einsum("bnyx,nc->bcyx", g_shift, wt[:, :, ky, kx])
            x_shift = xp[:, :, py + oy : py + oy + h, px + ox : px + ox + w]  # x[b, c, y + oy, x + ox]
            dw[:, :, ky, kx] = torch.einsum("bnyx,bcyx->nc", g, x_shift)
    return dx, dw, g.sum(dim=(0, 2, 3))


def backward64(grad_out, x, weight):
    """(dx, dw, db) in float64 by the closed form above."""
    return _sums(grad_out, x, weight, False)


def bounds64(grad_out, x, weight):
    """The same sums on absolute values: the operand magnitudes the fp32 rounding error of each element scales with."""
    return _sums(grad_out, x, weight, True)


def tolerances(case: Case, k: float = K):
    """Per-element (tol_x, tol_w, tol_b) = min(k, n + 2) * U * bound."""
    return tuple(min(k, n + 2) * U * bd for n, bd in zip(term_counts(case), bounds64(*case[1:])))


_REFERENCES = {}


def reference(case: Case):
    """((dx, dw, db), (tol_x, tol_w, tol_b), (bound_x, bound_w, bound_b)) of a committed case in float64, computed once
    per process."""
    if case.name not in _REFERENCES:
        _REFERENCES[case.name] = (backward64(*case[1:]), tolerances(case), bounds64(*case[1:]))
    return _REFERENCES[case.name]


def error_ratios(got_x, got_w, got_b, case: Case) -> Tuple[float, float, float]:
    """Worst error of each gradient in units of U * bound: what K has to cover. Elements whose bound is 0 must be
    exact."""
    refs, _, bounds = reference(case)
    out = []
    for got, ref, bd in zip((got_x, got_w, got_b), refs, bounds):
        err = (got.detach().cpu().double() - ref).abs()
        assert bool((err[bd == 0] == 0).all()), case.name
        live = bd > 0
        out.append(float((err[live] / (U * bd[live])).max()) if bool(live.any()) else 0.0)
    return tuple(out)


def assert_close(got_x: Optional[torch.Tensor], got_w: Optional[torch.Tensor], got_b: Optional[torch.Tensor], case: Case,
                 what: str) -> None:
    """Each given gradient (None: not checked) within its tolerance of float64, element by element; an element whose
    bound is 0 has tolerance 0 and must be exactly 0."""
    refs, tols, _ = reference(case)
    for name, got, ref, tol in zip(("grad_x", "grad_weight", "grad_bias"), (got_x, got_w, got_b), refs, tols):
        if got is None:
            continue
        assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float32, (what, case.name, name, got.shape)
        got = got.detach().cpu().double()
        assert bool(torch.isfinite(got).all()), (what, case.name, name, "not finite")
        err = (got - ref).abs()
        worst = float((err / tol.clamp(min=1e-300)).max())
        print(f"{what} {case.name} {name}: max |err| = {float(err.max()):.3e}, worst err / tol = {worst:.3f}")
        assert bool((err <= tol).all()), (what, case.name, name, worst)
