"""Float64 closed forms, error bounds and deterministic inputs of the batch-statistics batch norm tests
(csrc/batch_norm.hip: forward and backward, each with the ReLU after the layer folded in). PyTorch on the CPU only;
inputs come from seeded ``torch.Generator``s, so every machine rebuilds them bit for bit. Not a test module.

Per channel c over the n = B * H * W elements of (B, H, W): mean, var (biased), r = 1 / sqrt(var + eps),
xh = (x - mean) * r, y = xh * gamma + beta (through a ReLU when ``relu``); g = gy * [y > 0] with the ReLU, g = gy without:
    dbeta = sum g,   dgamma = sum g * xh,   dx = gamma * r * (g - dbeta / n - xh * dgamma / n)
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Tuple

import torch

from encoder_backward_cases import EPS, GRAD_SIGMA, RELU_GAP, U, _assert_close, gaussian

CHUNK = 8192  # csrc/batch_norm.hip: kChunk, the elements of a plane one workgroup sweeps (oflow_batch_norm_chunk_elements())


def workspace_floats(b: int, c: int, hw: int) -> int:
    """oflow_batch_norm_workspace_floats: two fp64 partials per (plane, chunk) and two fp64 sums per channel."""
    return 4 * b * c * ((hw + CHUNK - 1) // CHUNK) + 4 * c


# Tolerance per element: K * U * bound, bound the closed form on absolute values plus the conditioning term: rounding
# the mean to fp32 moves every x - mean by up to |mean| * U, i.e. xh by cond * U with cond = |mean| * r. With
# S1 = sum |g|, S2 = sum |g| |xh|:
#     y:      (|x - mean| + |mean|) * r * |gamma| + |beta|
#     mean:   sum |x| / n
#     var:    var + 2 |mean| * sum |x - mean| / n        (a constant channel: 0, so its variance must be exactly 0)
#     dbeta:  S1
#     dgamma: S2 + cond * S1
#     dx:     |gamma| r (|g| + S1 / n + |xh| S2 / n) + |gamma| r cond (S2 / n + |xh| S1 / n)
# One constant each for the output, the statistics and the gradients, four times what ATen's own fp32 CPU computation
# needs on BN_CASES: F.batch_norm(training=True) + relu for the output, its autograd for the gradients, and for the
# statistics what that call leaves in zero-initialised running buffers at momentum 1 (the mean; the unbiased variance,
# taken back to the biased one by (n - 1) / n in float64). tests/test_batch_norm_host.py::
# test_reference_fp32_calibrates_the_tolerances measures the ratios and asserts that they stay within K / 4. Measured
# maxima in units of U * bound: y 1.73 (2x64x12x20-relu); var 1.02 (1x2x16x16-relu), mean 0.004 (2x1x46x62-offset-relu;
# the other cases' means are 0 to rounding, so nothing is measured there: an fp32 result costs up to 0.5); dx 2.57
# (2x2x1x8197-relu), dgamma 0.78 (1x2x1x2-relu), dbeta 0.58 (2x64x12x20-relu). Each group's maximum is rounded up to
# the next multiple of 0.5 that leaves at least a quarter of headroom (the thread count and the vector width of the
# CPU change ATen's summation order; 1, 4 and 16 threads gave the same maxima): 2.5, 1.5 and 3.5, then times four.
#
# The ReLU's derivative jumps at 0. As in encoder_backward_cases.py the inputs keep every float64 pre-ReLU output at
# least RELU_GAP away from 0 (the host test asserts it), far above the forward's rounding error there (at most 1e-4: the
# offset case's cond * U = 6e-5).
K_OUT = 10.0
K_STAT = 6.0
K_GRAD = 14.0


class BNCase(NamedTuple):
    name: str
    relu: bool
    grad_out: torch.Tensor  # (B, C, H, W) fp32
    x: torch.Tensor  # (B, C, H, W) fp32
    weight: torch.Tensor  # (C,) fp32
    bias: torch.Tensor  # (C,) fp32

    @property
    def dims(self) -> Tuple[int, int, int]:
        """(B, C, HW): the C ABI's extents."""
        b, c, h, w = self.x.shape
        return b, c, h * w


# (B, C, H, W)
BN_SHAPES = [
    (1, 2, 1, 2),  # two elements per channel
    (2, 2, 7, 9),  # 63 = 4 * 15 + 3: planes start at every 16-byte phase
    (3, 3, 5, 7),  # 35 = 4 * 8 + 3, three planes per channel
    (1, 2, 15, 17),  # 255: one below the workgroup's thread count,
    (1, 2, 16, 16),  # 256,
    (1, 2, 1, 257),  # 257
    (2, 64, 12, 20),  # a real layer at reduced extent
    (2, 2, 1, CHUNK + 5),  # two chunks per plane, the second ragged (5 elements; 8197 is odd: unaligned second planes)
]
CONSTANT_SHAPE = (2, 2, 4, 8)  # channel 1 constant: 0.5 over 64 elements keeps an fp32 mean exact
OFFSET_SHAPE = (2, 1, 46, 62)  # mean 100, sigma 0.1: |mean| >> sigma


def make_case(shape, relu: bool, variant: str = "") -> BNCase:
    b, c, h, w = shape
    seed = 5000011 + 10007 * b + 101 * c + 37 * h + w
    v = lambda t: t.view(1, c, 1, 1)  # noqa: E731
    g = gaussian(seed + 3, shape, GRAD_SIGMA)
    gamma = gaussian(seed + 4, (c,)).double().abs() + 0.25
    gamma[0] = -gamma[0]  # a negative scale: the ReLU mask depends on the affine, not on the sign of x - mean
    beta = 0.5 * gaussian(seed + 5, (c,)).double()
    if variant == "constant":
        beta[1] = -0.3  # the constant channel's output is beta: below the gap, so its mask is empty
    gamma, beta = gamma.float(), beta.float()
    # The wanted output z = xh * gamma + beta must stay out of (-2 RELU_GAP, 2 RELU_GAP): xh out of the interval of
    # half-width 2 RELU_GAP / |gamma| around -beta / gamma. xh has mean 0 and variance 1 per channel by construction, so:
    # standardise per channel, push out of the interval, repeat (each push moves the statistics a little less).
    centre, half = v(-beta.double() / gamma.double()), v(2 * RELU_GAP / gamma.double().abs())
    t = gaussian(seed + 1, shape).double()
    for _ in range(12):
        t = t - t.mean(dim=(0, 2, 3), keepdim=True)
        t = t / torch.sqrt((t * t).mean(dim=(0, 2, 3), keepdim=True))
        t = torch.where(t >= centre, torch.maximum(t, centre + half), torch.minimum(t, centre - half))
    x = t
    if variant == "offset":
        x = 100.0 + 0.1 * t
    if variant == "constant":
        x = t.clone()
        x[:, 1] = 0.5
    name = f"{b}x{c}x{h}x{w}" + (f"-{variant}" if variant else "") + ("-relu" if relu else "")
    return BNCase(name, relu, g, x.float(), gamma, beta)


BN_CASES: List[BNCase] = []
for _relu in (True, False):
    BN_CASES += [make_case(sh, _relu) for sh in BN_SHAPES]
    BN_CASES += [make_case(CONSTANT_SHAPE, _relu, "constant"), make_case(OFFSET_SHAPE, _relu, "offset")]
BN_IDS = [c.name for c in BN_CASES]
BN_BY_NAME: Dict[str, BNCase] = dict(zip(BN_IDS, BN_CASES))
TWO_CHUNKS = f"2x2x1x{CHUNK + 5}-relu"
NAMES = ("y", "mean", "var", "grad_x", "grad_weight", "grad_bias")
KS = (K_OUT, K_STAT, K_STAT, K_GRAD, K_GRAD, K_GRAD)


def _stats64(case: BNCase):
    x = case.x.double()
    mean = x.mean(dim=(0, 2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
    return x, mean, var, 1.0 / torch.sqrt(var + EPS)


def output64(case: BNCase) -> torch.Tensor:
    """The layer's output before the ReLU, in float64."""
    x, mean, _, r = _stats64(case)
    c = x.shape[1]
    return (x - mean) * r * case.weight.double().view(1, c, 1, 1) + case.bias.double().view(1, c, 1, 1)


def _closed_forms(case: BNCase, absolute: bool):
    """(y, mean, var, dx, dgamma, dbeta) in float64, or their bounds."""
    x, mean, var, r = _stats64(case)
    c = x.shape[1]
    n = x.numel() // c
    gamma, beta = case.weight.double().view(1, c, 1, 1), case.bias.double().view(1, c, 1, 1)
    pre = (x - mean) * r * gamma + beta
    g = case.grad_out.double()
    if case.relu:
        g = g * (pre > 0)
    xh = (x - mean) * r
    csum = lambda t: t.sum(dim=(0, 2, 3), keepdim=True)  # noqa: E731
    if not absolute:
        y = torch.relu(pre) if case.relu else pre
        dbeta, dgamma = csum(g), csum(g * xh)
        dx = gamma * r * (g - dbeta / n - xh * dgamma / n)
        return y, mean.flatten(), var.flatten(), dx, dgamma.flatten(), dbeta.flatten()
    ga, xa, cond = g.abs(), xh.abs(), mean.abs() * r
    s1, s2 = csum(ga), csum(ga * xa)
    y = ((x - mean).abs() + mean.abs()) * r * gamma.abs() + beta.abs()
    bvar = var + 2 * mean.abs() * csum((x - mean).abs()) / n
    dx = gamma.abs() * r * (ga + s1 / n + xa * s2 / n) + gamma.abs() * r * cond * (s2 / n + xa * s1 / n)
    return y, (csum(x.abs()) / n).flatten(), bvar.flatten(), dx, (s2 + cond * s1).flatten(), s1.flatten()


_REFS = {}


def reference(case: BNCase):
    """(values, tolerances, bounds), each (y, mean, var, dx, dgamma, dbeta) in float64, computed once per process."""
    if case.name not in _REFS:
        bounds = _closed_forms(case, True)
        _REFS[case.name] = (_closed_forms(case, False), tuple(k * U * bd for k, bd in zip(KS, bounds)), bounds)
    return _REFS[case.name]


def error_ratios(gots, case: BNCase) -> Tuple[float, ...]:
    """Worst error of each of (y, mean, var, dx, dgamma, dbeta) in units of U * bound (None: skipped, 0.0); elements
    whose bound is 0 must be exact."""
    refs, _, bounds = reference(case)
    out = []
    for got, ref, bd in zip(gots, refs, bounds):
        if got is None:
            out.append(0.0)
            continue
        err = (got.detach().cpu().double() - ref).abs()
        assert bool((err[bd == 0] == 0).all()), case.name
        live = bd > 0
        out.append(float((err[live] / (U * bd[live])).max()) if bool(live.any()) else 0.0)
    return tuple(out)


def assert_close(gots, case: BNCase, what: str) -> None:
    """``gots``: (y, mean, var, dx, dgamma, dbeta), None for one not checked; each within K * U * bound of float64,
    element by element (an element whose bound is 0 must be exact)."""
    refs, tols, _ = reference(case)
    _assert_close(NAMES, tuple(gots), refs, tols, what, case.name)


def updated_buffers(running_mean, running_var, tracked, mean, var, n: int, momentum: float):
    """nn.BatchNorm2d's buffers after one train-mode call, from the batch's mean and biased variance (the formula
    model.extractor.enc_norm_act applies): the running variance takes the unbiased estimate var * n / (n - 1)."""
    return ((1 - momentum) * running_mean + momentum * mean,
            (1 - momentum) * running_var + momentum * var * n / (n - 1), tracked + 1)
