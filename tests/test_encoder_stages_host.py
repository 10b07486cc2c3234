"""The float64 references of the encoder-stage GPU tests (tests/encoder_stage_cases.py) checked on the CPU against the
real nn.Modules (model/extractor.py: ResidualBlock, BasicEncoder) and plain strided convolutions, so the GPU tests
compare the kernels with something that is itself pinned down. No GPU needed."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

import encoder_stage_cases as ec
from model.extractor import _fold_bn, _s2d_weight


def _rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------ 1a
@pytest.mark.parametrize("b,c,n,h,w", ec.S2D_HOST_CASES)
def test_space_to_depth_conv_equals_the_strided_conv(b, c, n, h, w):
    """_s2d_weight: the 2x2 convolution over the space-to-depth tensor (padded one row above, one column left) is the
    3x3 / stride 2 / pad 1 convolution to 1e-12 relative (the same products, summed in another order), and the 1x1
    shortcut over the first C channels is the 1x1 / stride 2 convolution exactly; the layout itself against its index
    formula, channel (a*2 + b)*C + c = pixel (2Y + a, 2X + b)."""
    g = ec.gen(100 + c + h)
    x = torch.randn(b, c, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    wt = torch.randn(n, c, 3, 3, generator=g, dtype=torch.float64)
    bias = torch.randn(n, generator=g, dtype=torch.float64)
    wd = torch.randn(n, c, 1, 1, generator=g, dtype=torch.float64)
    xs = ec.space_to_depth(x)
    assert xs.shape == (b, 4 * c, h, w)
    for a in range(2):
        for bb in range(2):
            for ch in (0, c - 1):
                for yy, xx in ((0, 0), (h - 1, w - 1)):
                    assert xs[b - 1, (a * 2 + bb) * c + ch, yy, xx] == x[b - 1, ch, 2 * yy + a, 2 * xx + bb]
    ref = F.conv2d(x, wt, bias, stride=2, padding=1)
    got = ec.conv_s2d64(xs, wt, bias)
    assert got.shape == ref.shape
    assert _rel(got, ref) <= 1e-12
    # the weight tensor itself: 9 of its 16 (quadrant, tap) slots hold the 3x3 taps, the other 7 are structural zeros
    w2 = _s2d_weight(wt).view(n, 4, c, 2, 2)
    assert int((w2 != 0).sum()) == int((wt != 0).sum())
    assert torch.equal(w2[:, 0, :, 1, 1], wt[:, :, 1, 1]) and torch.equal(w2[:, 3, :, 0, 0], wt[:, :, 0, 0])
    assert torch.equal(ec.shortcut_s2d64(xs, wd), F.conv2d(x, wd, stride=2))


@pytest.mark.parametrize("ky,kx", [(ky, kx) for ky in range(3) for kx in range(3)])
def test_shifted_tap_is_the_single_tap_strided_conv(ky, kx):
    g = ec.gen(7)
    x = torch.randint(-8, 9, (2, 10, 14), generator=g).double()
    wt = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    wt[0, 0, ky, kx] = 1
    assert torch.equal(ec.shifted_tap(x, ky, kx), F.conv2d(x[:, None], wt, stride=2, padding=1)[:, 0])


# ------------------------------------------------------------------------------------------------------------ 1b
@pytest.mark.parametrize("norm,stride,cin,n,b,h,w", ec.BLOCK_HOST_CASES)
def test_residual_block64_equals_the_module(norm, stride, cin, n, b, h, w):
    """norm_apply64 (every residual mode the encoder uses) composed with float64 convolutions -- for stride 2 in their
    space-to-depth form -- is ResidualBlock.double() to 1e-10 relative: instance norm from each conv output's own
    biased statistics (eps 1e-5), batch norm (eval, randomised running statistics and affine) folded into the convs.
    The fold runs in float64 (fold_bn64); extractor._fold_bn is that fold rounded once to fp32, checked bit for bit
    (its rounded weights alone move the block's output by ~1e-7, so they cannot meet 1e-10 themselves)."""
    blk = ec.host_block(norm, stride, cin, n, seed=40 + stride + n)
    x = torch.randn(b, cin, h, w, generator=ec.gen(5 + h), dtype=torch.float64)
    with torch.no_grad():
        ref = blk.double()(x.clone())
        got = ec.residual_block64(blk, x, norm)
    assert got.shape == ref.shape
    assert float(ref.abs().max()) > 0.1 and float((ref == 0).double().mean()) < 0.9
    assert _rel(got, ref) <= 1e-10
    if norm == "batch":
        pairs = [(blk.conv1, blk.norm1), (blk.conv2, blk.norm2)]
        if stride != 1:
            pairs.append((blk.downsample[0], blk.downsample[1]))
        for conv, bn in pairs:
            w64, b64 = ec.fold_bn64(conv, bn)
            w32, b32 = _fold_bn(conv, bn)
            assert w32.dtype == torch.float32 and torch.equal(w32, w64.float()) and torch.equal(b32, b64.float())


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("s2d", [False, True])
def test_norm_apply64_formulas(mode, s2d):
    """norm_apply64 against the formulas written out element by element, the space-to-depth order included."""
    g = ec.gen(20 + mode)
    b, c, h, w = 2, 8, 4, 6
    x, res, x2 = (torch.randn(b, c, h, w, generator=g, dtype=torch.float64) for _ in range(3))
    al, be, al2, be2 = (torch.randn(b, c, generator=g, dtype=torch.float64) for _ in range(4))
    y, mag = ec.norm_apply64(x, al, be, "relu", mode, res=res, x2=x2, alpha2=al2, beta2=be2, res_act="relu", s2d=s2d)
    for bi, ci, yy, xx in [(0, 0, 0, 0), (1, 7, 3, 5), (1, 3, 2, 1), (0, 5, 1, 4)]:
        v = max(float(x[bi, ci, yy, xx] * al[bi, ci] + be[bi, ci]), 0.0)
        if mode == 1:
            v = max(v + float(res[bi, ci, yy, xx]), 0.0)
        elif mode >= 2:
            r = float(x2[bi, ci, yy, xx] * al2[bi, ci] + be2[bi, ci])
            v = max(v + (max(r, 0.0) if mode == 3 else r), 0.0)
        got = y[bi, ((yy & 1) * 2 + (xx & 1)) * c + ci, yy >> 1, xx >> 1] if s2d else y[bi, ci, yy, xx]
        assert abs(float(got) - v) <= 1e-15 * max(1.0, abs(v))
    assert mag.shape == y.shape and bool((mag >= 0).all())


# ------------------------------------------------------------------------------------------------------------ 1c
@pytest.mark.parametrize("tiles", ec.STATS_HOST_TILES)
def test_merge64_equals_the_statistics_of_the_concatenated_samples(tiles):
    """merge64 of float64 (count, mean, M2) partials -- terms n, n*mean, M2 + n*mean^2 -- is the mean and the biased
    variance of the concatenated samples, over the regime norm_stats_kernel's comment assumes (mean^2 / var <= 1e4),
    the mean-100 / std-1.01 channel included. Bound: Q/N - mean^2 cancels, so each of its roundings (the sums S and Q,
    S/N, mean^2 with twice the mean's error, Q/N, the difference: 8 counted) costs 2^-53 * (mean^2 + var):
        |var - var_ref| <= 8 * 2^-53 * (mean^2 + var_ref),   |mean - mean_ref| <= 1e-12 * max(|mean_ref|, std).
    That is below 1e-12 * var wherever mean^2 / var <= 1.1e3 (asserted for every such channel); at the regime's edge,
    1e4, it is 8.9e-12 -- a flat 1e-12 there does not hold (this reference measures 1.5e-12 to 2.1e-12 on the mean-100
    channel), and alpha = 1/sqrt(var + eps) still has 4e-12, far below its fp32 rounding. For the constant channel
    (var = 0) the merged variance is below 1e-12 * mean^2."""
    b, c = 2, 12
    x, lens = ec.stats_samples(b, c, tiles, seed=300 + tiles)
    n, mean, m2 = ec.partials64(x, lens)
    assert n.shape == (b, tiles, c) and int(n[0, :, 0].sum()) == x.shape[2]
    mu, var = ec.merge64(n, mean, m2, dim=1)
    # two-pass reference (pairwise sums of centred squares: ~3e-16 relative; Tensor.var's Welford update has ~1e-14)
    mu_ref = x.mean(dim=2)
    var_ref = ((x - mu_ref[:, :, None]) ** 2).mean(dim=2)
    ok = mu_ref ** 2 <= 1e4 * var_ref
    assert x.shape[2] > 1 and bool(ok[:, 1:].all())
    assert bool(((mu - mu_ref).abs() <= 1e-12 * mu_ref.abs().clamp_min(var_ref.sqrt()))[ok].all())
    err = (var - var_ref).abs()
    assert bool((err <= 8 * 2.0 ** -53 * (mu_ref ** 2 + var_ref))[ok].all()), float((err / var_ref)[ok].max())
    mild = ok & (mu_ref ** 2 <= 1.1e3 * var_ref)
    assert bool(mild[:, 2:].all()) and bool((err <= 1e-12 * var_ref)[mild].all())
    assert bool((var[:, 0] <= 1e-12 * 0.75 ** 2).all())


def test_stats_partials_layout():
    part = ec.stats_partials_f32(2, 8, 32, 17, seed=1)
    assert part.shape == (2, 17, 32, 3) and part.dtype == torch.float32
    assert bool(torch.isfinite(part[:, :, :8]).all()) and bool(torch.isnan(part[:, :, 8:]).all())
    assert bool((part[:, :, 0, 2] == 0).all()) and bool((part[:, :, 0, 1] == 0.75).all())
    a, bb, mmax = ec.stats_reference(part, 8)
    assert float((a[:, 0] - 1e-5 ** -0.5).abs().max()) <= 1e-9
    assert float((part[:, :, 1, 1].double().mean() - 100).abs()) < 1.0 and float(mmax[:, 2].max()) < 3.0


# ------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("norm", ["instance", "batch"])
@pytest.mark.parametrize("shape", ec.ENCODER_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_encoder_cases_are_well_conditioned(norm, shape):
    """The whole-encoder cases: the fp32 module's own error against its float64 copy, e32, is positive and at most
    1e-4 * max |ref| -- the yardstick the GPU test holds SplitEncoder to is fp32 noise on well-conditioned inputs."""
    x, ref, e32 = ec.encoder_case(norm, shape)
    scale = float(ref.abs().max())
    print(f"{norm} {shape}: e32 {e32:.2e} at max |ref| {scale:.2f}")
    assert ref.shape == (shape[0], 256, shape[2] // 8, shape[3] // 8)
    assert 0.0 < e32 <= 1e-4 * scale
