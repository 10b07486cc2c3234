"""Float64 closed forms, error bounds and deterministic inputs of the encoder backward tests: the strided convolution
backward (csrc/conv_backward.hip) and the norm-layer backward (csrc/norm_backward.hip). PyTorch on the CPU only; inputs
come from seeded ``torch.Generator``s, so every machine rebuilds them bit for bit. Not a test module.

Convolution, stride s in {1, 2} (the same in y and x), zero padding (py, px) = (kh // 2, kw // 2), odd kh, kw, output
H' = (H + s - 1) // s, W' likewise. With out-of-image terms zero:
    dx[b, c, y, x]   = sum gy[b, n, Y, X] * w[n, c, ky, kx]   over (ky, kx, n) with s Y = y + py - ky, s X = x + px - kx
    dw[n, c, ky, kx] = sum_{b, Y, X} gy[b, n, Y, X] * x[b, c, s Y + ky - py, s X + kx - px]        n_w = B * H' * W' terms
    db[n]            = sum_{b, Y, X} gy[b, n, Y, X]                                                n_b = B * H' * W' terms
An input pixel meets at most ceil(kh / s) * ceil(kw / s) taps: n_x = that times Cout.

Norm layers, per plane (b, c) of HW elements, mu the mean, r = 1 / sqrt(var_biased + eps), xh = (x - mu) * r; with the
fused ReLU g = gy * [output > 0], without it g = gy:
    instance norm without affine:  dx = r * (g - mean(g) - xh * mean(g * xh))
    frozen batch norm:  y = (x - rm) * gamma / sqrt(rv + eps) + beta
        dx = g * gamma / sqrt(rv + eps),  dgamma = sum g * (x - rm) / sqrt(rv + eps),  dbeta = sum g    over (B, H, W)
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from conv_backward_cases import U, gaussian

# The kernels' tiling (csrc/conv_backward.hip: kCT, kWK, kSlab), which the shapes below are chosen around. At stride 2
# the dgrad tile holds 64 input pixels of one parity class and the wgrad chunks / slabs count OUTPUT pixels.
PIXEL_TILE = 64
K_CHUNK = 32
SLAB = 2048
FOLD_MAX_CIN = 4  # the strided weight gradient folds (channel, tap) into one tile dimension up to this Cin

# ---------------------------------------------------------------------------------------------------------------
# strided convolution
# ---------------------------------------------------------------------------------------------------------------
# Tolerance per element: min(K_CONV, n + 2) * U * bound (the rule of tests/conv_backward_cases.py). K_CONV is four times
# what ATen's own fp32 CPU autograd of F.conv2d(stride=2) needs on CONV_CASES
# (tests/test_encoder_backward_host.py::test_conv_reference_fp32_autograd_calibrates_the_tolerance measures it and
# asserts it stays within K_CONV / 4). Measured maxima over the committed cases, in units of U * bound: dx 4.84
# (3x3-c8-n8-3x81x73-s2), dw 4.68 (3x3-c96-n128-2x12x20-s2), db 1.78 (3x3-c33-n126-2x4x7-s2). Rounded up to 5.5 as
# conv_backward_cases.py does (the CPU's thread count and vector width change ATen's summation order), then times four.
K_CONV = 22.0


class ConvCase(NamedTuple):
    name: str
    grad_out: torch.Tensor  # (B, Cout, H', W') fp32
    x: torch.Tensor  # (B, Cin, H, W) fp32
    weight: torch.Tensor  # (Cout, Cin, kh, kw) fp32
    stride: int

    @property
    def dims(self) -> Tuple[int, ...]:
        """(B, Cout, Cin, H, W, kh, kw, stride): the strided C ABI's argument order."""
        b, cin, h, w = self.x.shape
        cout, _, kh, kw = self.weight.shape
        return b, cout, cin, h, w, kh, kw, self.stride


# (kh, kw, Cin, Cout, B, H, W), all at stride 2
CONV_SHAPES = [
    (3, 3, 5, 6, 1, 1, 1),  # images smaller than the kernel: taps leave on every side
    (3, 3, 5, 6, 1, 2, 2),
    (3, 3, 5, 6, 2, 5, 5),
    (7, 7, 5, 6, 1, 1, 1),
    (7, 7, 5, 6, 1, 2, 2),
    (7, 7, 5, 6, 2, 5, 5),
    (3, 3, 33, 126, 2, 4, 8),  # even sizes; channels one past the 32-lane tile / two short of two tiles
    (3, 3, 33, 126, 3, 5, 7),  # odd sizes: the ceil output size
    (3, 3, 33, 126, 2, 4, 7),  # mixed
    (1, 1, 33, 33, 2, 5, 7),  # the 1x1 projection: three parity classes of dx are exact zeros
    (3, 3, 8, 8, 3, 3, 7),  # 63 input pixels over three images
    (3, 3, 8, 8, 5, 1, 13),  # 65 input pixels over five images (64: 2x4x8 above)
    (3, 3, 8, 8, 3, 5, 13),  # 63 pixels in the largest parity class: one below the dgrad tile
    (3, 3, 8, 8, 1, 16, 16),  # 64 in every class: exactly one tile
    (3, 3, 8, 8, 5, 1, 26),  # 65 in each of the two classes a one-row image has: one past the tile
    (3, 3, 8, 8, 2, 8, 8),  # 32 output pixels: one wgrad K chunk
    (3, 3, 8, 8, 3, 1, 22),  # 33 output pixels: one past it
    (3, 3, 8, 8, 2, 64, 64),  # 2048 output pixels: exactly one slab
    (3, 3, 8, 8, 1, 1, 4097),  # 2049: a second slab of one pixel
    (3, 3, 8, 8, 3, 81, 73),  # 3 x 41 x 37 = 4551: two full slabs and a remainder, the slab edges inside images
    (7, 7, 3, 64, 2, 9, 10),  # the stem: the folded Cin <= 4 weight gradient (147 columns = 3 tiles, the last ragged)
    (7, 7, 3, 64, 2, 16, 24),
    (7, 7, 4, 33, 2, 9, 10),  # the largest folded Cin; compared with its zero-padded c5 twin on the generic path
    (3, 3, 64, 96, 2, 12, 20),  # the real layers at reduced extent: layer2's first conv,
    (3, 3, 96, 128, 2, 12, 20),  # layer3's,
    (1, 1, 64, 96, 2, 12, 20),  # and layer2's projection
]
GRAD_SIGMA = 1e-3
WEIGHT_SIGMA = 0.1


def out_size(n: int, s: int) -> int:
    return (n + s - 1) // s


def make_conv_case(shape, stride: int = 2, single: bool = False) -> ConvCase:
    kh, kw, cin, cout, b, h, w = shape
    seed = 2000003 * (kh * 8 + kw) + 10007 * cin + 101 * cout + 1009 * b + 37 * h + w + 7 * stride
    ho, wo = out_size(h, stride), out_size(w, stride)
    x = gaussian(seed + 1, (b, cin, h, w))
    wt = gaussian(seed + 2, (cout, cin, kh, kw), WEIGHT_SIGMA)
    g = gaussian(seed + 3, (b, cout, ho, wo), GRAD_SIGMA)
    name = f"{kh}x{kw}-c{cin}-n{cout}-{b}x{h}x{w}-s{stride}"
    if single:  # zero except at output pixel (ho // 2, wo // 2) of the last image: most input gradients are exactly 0
        one = torch.zeros_like(g)
        one[b - 1, :, ho // 2, wo // 2] = g[b - 1, :, ho // 2, wo // 2]
        g, name = one, name + "-single"
    return ConvCase(name, g, x, wt, stride)


CONV_CASES: List[ConvCase] = [make_conv_case(sh) for sh in CONV_SHAPES] + [
    make_conv_case((3, 3, 33, 33, 2, 5, 6), single=True)]
CONV_IDS = [c.name for c in CONV_CASES]
CONV_BY_NAME: Dict[str, ConvCase] = dict(zip(CONV_IDS, CONV_CASES))
# three of the shapes at stride 1 through the strided entry points: bit-identical to the stride-1 entry points
# (none with Cin <= 4, whose weight gradient takes the folded path)
STRIDE1_CASES: List[ConvCase] = [make_conv_case(sh, stride=1) for sh in
                                 ((3, 3, 33, 126, 2, 4, 8), (1, 1, 33, 33, 2, 5, 7), (3, 3, 8, 8, 3, 81, 73))]
STRIDE1_IDS = [c.name for c in STRIDE1_CASES]


def pad_channels(case: ConvCase, cin: int) -> ConvCase:
    """The same convolution with zero input channels (and zero weights for them) appended up to ``cin``."""
    b, c0, h, w = case.x.shape
    x = torch.cat([case.x, torch.zeros(b, cin - c0, h, w)], dim=1)
    wt = torch.cat([case.weight, torch.zeros(case.weight.shape[0], cin - c0, *case.weight.shape[2:])], dim=1)
    return ConvCase(case.name + f"-padded-c{cin}", case.grad_out, x, wt, case.stride)


def conv_term_counts(case: ConvCase) -> Tuple[int, int, int]:
    """(n_x, n_w, n_b): the largest number of terms of one element's sum."""
    b, cout, _, h, w, kh, kw, s = case.dims
    n_out = b * out_size(h, s) * out_size(w, s)
    return out_size(kh, s) * out_size(kw, s) * cout, n_out, n_out


def _tap_slices(n: int, k: int, tap: int, s: int):
    """Output indices Y and input indices y = s Y + tap - k // 2 inside [0, n), as two slices (None: no such pair)."""
    p, no = k // 2, out_size(n, s)
    lo = max(0, -((tap - p) // s))  # the smallest Y with s Y + tap - p >= 0
    hi = min(no - 1, (n - 1 - tap + p) // s)  # the largest with s Y + tap - p <= n - 1
    if hi < lo:
        return None
    return slice(lo, hi + 1), slice(s * lo + tap - p, s * hi + tap - p + 1, s)


def _conv_sums(grad_out, x, weight, stride: int, absolute: bool):
    g, xs, wt = grad_out.double(), x.double(), weight.double()
    if absolute:
        g, xs, wt = g.abs(), xs.abs(), wt.abs()
    h, w = xs.shape[-2:]
    kh, kw = wt.shape[-2:]
    dx, dw = torch.zeros_like(xs), torch.zeros_like(wt)
    for ky in range(kh):
        ys = _tap_slices(h, kh, ky, stride)
        for kx in range(kw):
            xsl = _tap_slices(w, kw, kx, stride)
            if ys is None or xsl is None:
                continue
            gs = g[:, :, ys[0], xsl[0]]
            dx[:, :, ys[1], xsl[1]] += torch.einsum("bnyx,nc->bcyx", gs, wt[:, :, ky, kx])
            dw[:, :, ky, kx] = torch.einsum("bnyx,bcyx->nc", gs, xs[:, :, ys[1], xsl[1]])
    return dx, dw, g.sum(dim=(0, 2, 3))


def conv_backward64(case: ConvCase):
    """(dx, dw, db) in float64 by the closed form above."""
    return _conv_sums(case.grad_out, case.x, case.weight, case.stride, False)


def conv_bounds64(case: ConvCase):
    """The same sums on absolute values: the operand magnitudes the fp32 rounding error of each element scales with."""
    return _conv_sums(case.grad_out, case.x, case.weight, case.stride, True)


def conv_tolerances(case: ConvCase, k: float = K_CONV):
    return tuple(min(k, n + 2) * U * bd for n, bd in zip(conv_term_counts(case), conv_bounds64(case)))


_CONV_REFS = {}


def conv_reference(case: ConvCase):
    """((dx, dw, db), tolerances, bounds) in float64, computed once per process."""
    if case.name not in _CONV_REFS:
        _CONV_REFS[case.name] = (conv_backward64(case), conv_tolerances(case), conv_bounds64(case))
    return _CONV_REFS[case.name]


def _ratios(gots, refs, bounds, name) -> Tuple[float, ...]:
    out = []
    for got, ref, bd in zip(gots, refs, bounds):
        err = (got.detach().cpu().double() - ref).abs()
        assert bool((err[bd == 0] == 0).all()), name
        live = bd > 0
        out.append(float((err[live] / (U * bd[live])).max()) if bool(live.any()) else 0.0)
    return tuple(out)


def conv_error_ratios(got_x, got_w, got_b, case: ConvCase) -> Tuple[float, ...]:
    """Worst error of each gradient in units of U * bound: what K_CONV has to cover. Elements whose bound is 0 must be
    exact."""
    refs, _, bounds = conv_reference(case)
    return _ratios((got_x, got_w, got_b), refs, bounds, case.name)


def _assert_close(names, gots, refs, tols, what: str, case_name: str) -> None:
    for name, got, ref, tol in zip(names, gots, refs, tols):
        if got is None:
            continue
        assert tuple(got.shape) == tuple(ref.shape) and got.dtype == torch.float32, (what, case_name, name, got.shape)
        got = got.detach().cpu().double()
        assert bool(torch.isfinite(got).all()), (what, case_name, name, "not finite")
        err = (got - ref).abs()
        worst = float((err / tol.clamp(min=1e-300)).max()) if err.numel() else 0.0
        print(f"{what} {case_name} {name}: max |err| = {float(err.max()) if err.numel() else 0.0:.3e}, "
              f"worst err / tol = {worst:.3f}")
        assert bool((err <= tol).all()), (what, case_name, name, worst)


def assert_conv_close(got_x: Optional[torch.Tensor], got_w: Optional[torch.Tensor], got_b: Optional[torch.Tensor],
                      case: ConvCase, what: str) -> None:
    """Each given gradient (None: not checked) within its tolerance of float64, element by element; an element whose
    bound is 0 has tolerance 0 and must be exactly 0."""
    refs, tols, _ = conv_reference(case)
    _assert_close(("grad_x", "grad_weight", "grad_bias"), (got_x, got_w, got_b), refs, tols, what, case.name)


# ---------------------------------------------------------------------------------------------------------------
# norm layers
# ---------------------------------------------------------------------------------------------------------------
# Tolerance per element: K_NORM * U * bound. bound is the closed form on absolute values plus the conditioning term:
# rounding mu (or the running mean) to fp32 moves xh by up to |mu| * r * U, which the instance norm's
# dx = r * (g - mean(g) - xh * mean(g * xh)) sees as r * (|mu| r) * (mean|g xh| + |xh| mean|g|); the batch norm's dgamma
# sums |g| * (|x| + |rm|) * rstd instead of |g| * |x - rm| * rstd. K_NORM is four times what ATen's own fp32 CPU autograd
# of relu(F.instance_norm(x)) / F.batch_norm(training=False) needs on NORM_CASES
# (tests/test_encoder_backward_host.py::test_norm_reference_fp32_autograd_calibrates_the_tolerance measures it and
# asserts it stays within K_NORM / 4; planes of one element excepted, which F.instance_norm refuses). Measured maxima in
# units of U * bound: instance norm dx 2.40 (2x64x12x20, ReLU); frozen batch norm dx 2.60 (2x64x12x20, ReLU), dgamma
# 1.16 and dbeta 0.54 (1x2x1x2). Rounded up to 3.5 (the headroom conv_backward_cases.py takes), then times four.
#
# The ReLU's derivative jumps at 0, and an fp32 forward places an output within its rounding error of 0 on either side.
# The inputs therefore keep every pre-ReLU output at least RELU_GAP away from 0 (the host test asserts it), far above
# that rounding error (at most 1e-4 here: the offset plane's |mu| r U = 6e-5), and one plane is constant: there xh is
# exactly 0, the mask is empty and var = 0 (r = 1 / sqrt(eps)); its value 0.5 and size 64 keep an fp32 mean exact.
K_NORM = 14.0
EPS = 1e-5
RELU_GAP = 0.05


class NormCase(NamedTuple):
    name: str
    kind: str  # "instance" | "frozen_bn"
    relu: bool
    grad_out: torch.Tensor  # (B, C, H, W) fp32
    x: torch.Tensor  # (B, C, H, W) fp32
    weight: Optional[torch.Tensor]  # frozen_bn: (C,) each
    bias: Optional[torch.Tensor]
    running_mean: Optional[torch.Tensor]
    running_var: Optional[torch.Tensor]


# (B, C, H, W)
NORM_SHAPES = [
    (1, 2, 1, 1),  # planes of 1 element,
    (1, 2, 1, 2),  # 2,
    (2, 2, 7, 9),  # 63 = 4 * 15 + 3: planes start at every 16-byte phase,
    (1, 3, 8, 8),  # 64,
    (1, 2, 5, 13),  # 65 = 4 * 16 + 1,
    (1, 2, 15, 17),  # 255: one below the workgroup's thread count,
    (1, 2, 16, 16),  # 256,
    (1, 2, 1, 257),  # 257
    (2, 3, 5, 7),  # 35 = 4 * 8 + 3
    (2, 64, 12, 20),  # a real layer at reduced extent
]
CONSTANT_SHAPE = (1, 2, 8, 8)  # plane (0, 0) constant
OFFSET_SHAPE = (2, 1, 46, 62)  # mean 100, sigma 0.1: |mu| >> sigma


def _gapped(seed: int, shape) -> torch.Tensor:
    """Standard normal values pushed out of (-2 RELU_GAP, 2 RELU_GAP): what the pre-ReLU output is built from."""
    z = gaussian(seed, shape).double()
    return torch.where(z >= 0, z.clamp(min=2 * RELU_GAP), z.clamp(max=-2 * RELU_GAP))


def make_norm_case(kind: str, shape, relu: bool, variant: str = "") -> NormCase:
    b, c, h, w = shape
    seed = 3000017 + 10007 * b + 101 * c + 37 * h + w + (5 if kind == "instance" else 11)
    g = gaussian(seed + 3, shape, GRAD_SIGMA)
    z = _gapped(seed + 1, shape)
    name = f"{kind}-{b}x{c}x{h}x{w}" + (f"-{variant}" if variant else "") + ("-relu" if relu else "")
    if kind == "instance":
        for _ in range(8):  # the output is relative to the plane's mean: centre, push out of the gap again, repeat
            z = z - z.mean(dim=(2, 3), keepdim=True)
            z = torch.where(z >= 0, z.clamp(min=2 * RELU_GAP), z.clamp(max=-2 * RELU_GAP))
        x = z
        if variant == "offset":
            x = 100.0 + 0.1 * z
        if variant == "constant":
            x = z.clone()
            x[0, 0] = 0.5
        return NormCase(name, kind, relu, g, x.float(), None, None, None, None)
    gamma = gaussian(seed + 4, (c,)).double().abs() + 0.25
    gamma[0] = -gamma[0]  # a negative scale: the ReLU mask depends on the affine, not on the sign of x - rm
    beta = 0.5 * gaussian(seed + 5, (c,)).double()
    rm = gaussian(seed + 6, (c,)).double()
    rv = torch.logspace(0.5, -6, c, dtype=torch.float64) if c > 1 else torch.tensor([1e-6], dtype=torch.float64)
    gamma, beta, rm, rv = (t.float() for t in (gamma, beta, rm, rv))
    # x such that the layer's output is z up to fp32 rounding (far below the gap)
    alpha = (gamma.double() / torch.sqrt(rv.double() + EPS)).view(1, c, 1, 1)
    x = rm.double().view(1, c, 1, 1) + (z - beta.double().view(1, c, 1, 1)) / alpha
    return NormCase(name, kind, relu, g, x.float(), gamma, beta, rm, rv)


NORM_CASES: List[NormCase] = []
for _kind in ("instance", "frozen_bn"):
    for _relu in (True, False):
        NORM_CASES += [make_norm_case(_kind, sh, _relu) for sh in NORM_SHAPES]
    NORM_CASES += [make_norm_case("instance", CONSTANT_SHAPE, r, "constant") for r in (True, False)] if _kind == "instance" else []
    NORM_CASES += [make_norm_case("instance", OFFSET_SHAPE, r, "offset") for r in (True, False)] if _kind == "instance" else []
NORM_IDS = [c.name for c in NORM_CASES]
NORM_BY_NAME: Dict[str, NormCase] = dict(zip(NORM_IDS, NORM_CASES))


def norm_output64(case: NormCase) -> torch.Tensor:
    """The layer's output before the ReLU, in float64."""
    x = case.x.double()
    if case.kind == "instance":
        mu = x.mean(dim=(2, 3), keepdim=True)
        var = ((x - mu) ** 2).mean(dim=(2, 3), keepdim=True)
        return (x - mu) / torch.sqrt(var + EPS)
    v = lambda t: t.double().view(1, -1, 1, 1)  # noqa: E731
    return (x - v(case.running_mean)) * v(case.weight) / torch.sqrt(v(case.running_var) + EPS) + v(case.bias)


def _norm_sums(case: NormCase, absolute: bool):
    x, g = case.x.double(), case.grad_out.double()
    if case.relu:
        g = g * (norm_output64(case) > 0)
    mean = lambda t: t.mean(dim=(2, 3), keepdim=True)  # noqa: E731
    if case.kind == "instance":
        mu = mean(x)
        r = 1.0 / torch.sqrt(mean((x - mu) ** 2) + EPS)
        xh = (x - mu) * r
        if not absolute:
            return (r * (g - mean(g) - xh * mean(g * xh)),)
        ga, xa = g.abs(), xh.abs()
        cond = mu.abs() * r
        return (r * (ga + mean(ga) + xa * mean(ga * xa)) + r * cond * (mean(ga * xa) + xa * mean(ga)),)
    v = lambda t: t.double().view(1, -1, 1, 1)  # noqa: E731
    rm, gamma = v(case.running_mean), v(case.weight)
    rstd = 1.0 / torch.sqrt(v(case.running_var) + EPS)
    if not absolute:
        return g * gamma * rstd, (g * (x - rm) * rstd).sum(dim=(0, 2, 3)), g.sum(dim=(0, 2, 3))
    ga = g.abs()
    return ga * gamma.abs() * rstd, (ga * (x.abs() + rm.abs()) * rstd).sum(dim=(0, 2, 3)), ga.sum(dim=(0, 2, 3))


def norm_backward64(case: NormCase):
    """(dx,) for the instance norm, (dx, dgamma, dbeta) for the frozen batch norm, in float64."""
    return _norm_sums(case, False)


def norm_bounds64(case: NormCase):
    return _norm_sums(case, True)


_NORM_REFS = {}


def norm_reference(case: NormCase):
    """(gradients, tolerances, bounds) in float64, computed once per process."""
    if case.name not in _NORM_REFS:
        bounds = norm_bounds64(case)
        _NORM_REFS[case.name] = (norm_backward64(case), tuple(K_NORM * U * bd for bd in bounds), bounds)
    return _NORM_REFS[case.name]


def norm_error_ratios(gots, case: NormCase) -> Tuple[float, ...]:
    refs, _, bounds = norm_reference(case)
    return _ratios(gots, refs, bounds, case.name)


def assert_norm_close(gots, case: NormCase, what: str) -> None:
    """``gots``: (dx,) or (dx, dgamma, dbeta), None for a gradient not checked; each within K_NORM * U * bound of float64,
    element by element (an element whose bound is 0 must be exactly 0)."""
    refs, tols, _ = norm_reference(case)
    _assert_close(("grad_x", "grad_weight", "grad_bias"), tuple(gots), refs, tols, what, case.name)
