"""Float64 references, deterministic inputs and case lists of the encoder-stage tests (csrc/encoder_s32.hip and the
convolution epilogues of csrc/conv_s32.hip that model/extractor.py's SplitEncoder uses): the space-to-depth form of the
stride-2 convolutions, the norm-apply kernel, the merge of the instance-norm partials, and the residual block composed
from them. PyTorch on the CPU only; inputs come from seeded ``torch.Generator``s or model/synthetic.py's hash images,
so every machine rebuilds them bit for bit. tests/test_encoder_stages_host.py pins these references against the real
``nn.Module``s; tests/test_gpu_encoder_stages.py compares the kernels with them. Not a test module."""
from __future__ import annotations

import copy
import functools
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from model import synthetic
from model.extractor import BasicEncoder, ResidualBlock, _fold_bn, _s2d_weight

EPS = 1e-5  # nn.InstanceNorm2d / nn.BatchNorm2d default

# ---------------------------------------------------------------------------------------------------- case lists
# 1a: (B, C, N, h, w) = stride-2 output size h x w of a (B, C, 2h, 2w) input
S2D_HOST_CASES = [(2, 8, 16, 5, 7), (1, 64, 96, 1, 1), (1, 96, 128, 4, 3)]
# 1b: (norm, stride, in_planes, planes, B, H, W)
BLOCK_HOST_CASES = [(norm, stride, cin, n, b, h, w)
                    for norm in ("instance", "batch")
                    for stride, cin, n, b, h, w in [(1, 16, 16, 2, 6, 10), (2, 8, 16, 2, 6, 10), (2, 16, 24, 1, 4, 34)]]

# 2: oflow_norm_stats_finalize. 16 waves stride over the tiles: one partial per wave up to 16 tiles, more from 17; the
# 4-in-flight loop (t + 48 < tiles) first runs at 49 tiles and its period is 64 tiles.
STATS_TILES = [1, 15, 16, 17, 48, 49, 63, 64, 65, 130, 257]
STATS_CHANNELS = [(8, 32), (64, 64), (96, 96), (130, 160)]  # (C, n_pad): one lane block, a full one, 1.5, n_pad > C
STATS_BATCH = [1, 3]
STATS_HOST_TILES = [1, 17, 65, 257]

# 3: oflow_norm_apply_s32
APPLY_SHAPES = [(1, 2, 2), (2, 6, 10), (3, 4, 34)]
APPLY_CHANNELS = [8, 40, 64, 96, 128]
# (res_mode, act, res_act, s2d): the pairs SplitEncoder issues ...
APPLY_ENCODER_MODES = [(0, "relu", "none", s) for s in (0, 1)] + [(m, "relu", "relu", s) for m in (1, 2, 3) for s in (0, 1)]
# ... and the rest of the cross product {0..3} x {none, relu}^2 x {0, 1}
APPLY_OTHER_MODES = [(m, a, ra, s) for m in range(4) for a in ("none", "relu") for ra in ("none", "relu") for s in (0, 1)
                     if (m, a, ra, s) not in APPLY_ENCODER_MODES]
APPLY_OTHER_C = 40
APPLY_CASES = ([(shape, c) + mode for shape in APPLY_SHAPES for c in APPLY_CHANNELS for mode in APPLY_ENCODER_MODES]
               + [(shape, APPLY_OTHER_C) + mode for shape in APPLY_SHAPES for mode in APPLY_OTHER_MODES])

# 4: the 3x3 convolutions of the batch-norm encoder's residual tails: (channels = block_n, (B, H, W), s2d)
RES_CONV_CASES = [(n, shape, s2d) for n in (64, 96, 128) for shape in [(2, 6, 34), (1, 4, 32), (1, 10, 70)] for s2d in (False, True)]

# 5: the stride-2 stage: (C, N = block_n) and output sizes (h, w); B = 2 everywhere (a batch boundary in every grid)
S2_CHANNELS = [(32, 64), (64, 96), (96, 128)]
S2_SIZES = [(1, 1), (4, 32), (5, 33), (9, 40)]
S2_BATCH = 2
SHORTCUT_CHANNELS = [(64, 96), (96, 128)]

# 6: whole encoder
ENCODER_SHAPES = [(2, 3, 24, 40), (1, 3, 16, 72), (3, 3, 40, 24)]
ENCODER_VARIANTS = ["plain", "split_out", "stem_from_image"]


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


# ------------------------------------------------------------------------------------------- space-to-depth (1a)
def space_to_depth(x: torch.Tensor) -> torch.Tensor:
    """(B, C, 2h, 2w) -> (B, 4C, h, w): channel (a*2 + b)*C + c of pixel (Y, X) is input pixel (2Y + a, 2X + b) of
    channel c. (Written out quadrant by quadrant: F.pixel_unshuffle orders the channels c*4 + a*2 + b.)"""
    b, c, hh, ww = x.shape
    assert hh % 2 == 0 and ww % 2 == 0
    out = x.new_empty((b, 4 * c, hh // 2, ww // 2))
    for a in range(2):
        for bb in range(2):
            q = a * 2 + bb
            out[:, q * c:(q + 1) * c] = x[:, :, a::2, bb::2]
    return out


def conv_s2d64(xs: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The 3x3 / stride 2 / pad 1 convolution with weights ``w`` (N, C, 3, 3) as SplitEncoder runs it: a 2x2 stride-1
    convolution with ``_s2d_weight(w)`` over the space-to-depth input ``xs``, taps at offsets -1 and 0 (one zero row
    above and one zero column left). float64."""
    w2 = _s2d_weight(w.double())
    return F.conv2d(F.pad(xs.double(), (1, 0, 1, 0)), w2, None if bias is None else bias.double())


def shortcut_s2d64(xs: torch.Tensor, wd: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The 1x1 / stride 2 shortcut: a 1x1 convolution over the first C channels (quadrant a = b = 0) of ``xs``."""
    c = wd.shape[1]
    return F.conv2d(xs[:, :c].double(), wd.double(), None if bias is None else bias.double())


# ------------------------------------------------------------------------------------------------ norm-apply (1b)
def act64(v: torch.Tensor, act) -> torch.Tensor:
    act = {0: "none", 1: "relu", 2: "sigmoid", 3: "tanh"}.get(act, act)
    return {"none": lambda t: t, "relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act](v)


def _bc(a: torch.Tensor) -> torch.Tensor:
    return a.double()[:, :, None, None]


def norm_apply64(x, alpha, beta, act="none", res_mode=0, res=None, x2=None, alpha2=None, beta2=None, res_act="none",
                 s2d=False) -> Tuple[torch.Tensor, torch.Tensor]:
    """oflow_norm_apply_s32 restated in float64 on (B, C, H, W) tensors with per-(image, channel) affines (B, C):
        y = act(x*alpha + beta)
        mode 1: y = res_act(y + res)                              (identity shortcut)
        mode 2: y = res_act(y + (x2*alpha2 + beta2))              (normalised downsample branch)
        mode 3: y = res_act(y + relu(x2*alpha2 + beta2))          (a block input kept raw)
    then, with ``s2d``, the space-to-depth layout of y. Returns (y, mag): mag = |x*alpha| + |beta| + |residual terms|,
    the magnitudes whose fp32 roundings bound the kernel's error (same layout as y)."""
    x = x.double()
    lin = x * _bc(alpha)
    y = act64(lin + _bc(beta), act)
    mag = lin.abs() + _bc(beta).abs()
    if res_mode == 1:
        y = act64(y + res.double(), res_act)
        mag = mag + res.double().abs()
    elif res_mode in (2, 3):
        lin2 = x2.double() * _bc(alpha2)
        r = lin2 + _bc(beta2)
        if res_mode == 3:
            r = torch.relu(r)
        y = act64(y + r, res_act)
        mag = mag + lin2.abs() + _bc(beta2).abs()
    else:
        assert res_mode == 0
    if s2d:
        y, mag = space_to_depth(y), space_to_depth(mag)
    return y, mag


def instance_affine64(y: torch.Tensor, eps: float = EPS) -> Tuple[torch.Tensor, torch.Tensor]:
    """nn.InstanceNorm2d (no affine, biased variance) of a conv output (B, C, H, W) as y*alpha + beta, float64."""
    y = y.double()
    mean = y.mean(dim=(2, 3))
    var = y.var(dim=(2, 3), unbiased=False)
    alpha = 1.0 / torch.sqrt(var + eps)
    return alpha, -mean * alpha


def fold_bn64(conv: nn.Conv2d, bn: nn.BatchNorm2d) -> Tuple[torch.Tensor, torch.Tensor]:
    """extractor._fold_bn without its final rounding to fp32: eval-mode batch norm folded into the conv, float64."""
    w = conv.weight.detach().double()
    b = conv.bias.detach().double()
    alpha = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    beta = bn.bias.detach().double() - bn.running_mean.detach().double() * alpha
    return w * alpha.view(-1, 1, 1, 1), b * alpha + beta


def randomise_bn(module: nn.Module, seed: int) -> None:
    """Non-trivial running statistics and affine parameters for every BatchNorm2d of ``module``."""
    g = gen(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)


def residual_block64(blk: ResidualBlock, x: torch.Tensor, norm: str, fold=fold_bn64) -> torch.Tensor:
    """A ResidualBlock forward in the order SplitEncoder executes it, from float64 convolutions and norm_apply64.
    Stride 2: conv1 and the shortcut read the space-to-depth input (conv_s2d64, shortcut_s2d64). Instance norm: each
    conv's raw output with its own statistics, the tail as residual mode 1 (identity) or 2 (norm3 of the shortcut).
    Batch norm (eval): folded into the convs by ``fold``; the tail is mode 1 on the folded shortcut's output."""
    x = x.double()
    s2 = blk.downsample is not None
    b = x.shape[0]
    ones = lambda n: torch.ones(b, n, dtype=torch.float64)
    zeros = lambda n: torch.zeros(b, n, dtype=torch.float64)

    def wb(conv, bn):
        if norm == "batch":
            w, bias = fold(conv, bn)
            return w.double(), bias.double()
        return conv.weight.detach().double(), conv.bias.detach().double()

    w1, b1 = wb(blk.conv1, blk.norm1)
    w2, b2 = wb(blk.conv2, blk.norm2)
    if s2:
        xs = space_to_depth(x)
        r1 = conv_s2d64(xs, w1, b1)
        wd, bd = wb(blk.downsample[0], blk.downsample[1])
        rd = shortcut_s2d64(xs, wd, bd)
    else:
        r1 = F.conv2d(x, w1, b1, padding=1)
    n = r1.shape[1]
    a1, be1 = instance_affine64(r1) if norm == "instance" else (ones(n), zeros(n))
    t, _ = norm_apply64(r1, a1, be1, "relu")
    r2 = F.conv2d(t, w2, b2, padding=1)
    a2, be2 = instance_affine64(r2) if norm == "instance" else (ones(n), zeros(n))
    if not s2:
        return norm_apply64(r2, a2, be2, "relu", 1, res=x, res_act="relu")[0]
    if norm == "instance":
        a3, be3 = instance_affine64(rd)
        return norm_apply64(r2, a2, be2, "relu", 2, x2=rd, alpha2=a3, beta2=be3, res_act="relu")[0]
    return norm_apply64(r2, a2, be2, "relu", 1, res=rd, res_act="relu")[0]


def host_block(norm: str, stride: int, cin: int, n: int, seed: int) -> ResidualBlock:
    torch.manual_seed(seed)
    blk = ResidualBlock(cin, n, norm, stride=stride).eval()
    if norm == "batch":
        randomise_bn(blk, seed + 1)
    return blk


# ----------------------------------------------------------------------------------- (count, mean, M2) merge (1c)
def merge64(n: torch.Tensor, mean: torch.Tensor, m2: torch.Tensor, dim: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Merge of (count, mean, M2) partials along ``dim`` as norm_stats_kernel does it: plain float64 sums of n, n*mean
    and M2 + n*mean^2; mean = S/N, biased variance = Q/N - mean^2 (clamped at 0). The difference cancels: the variance is
    accurate to a few 2^-53 * (1 + mean^2 / var) relative, i.e. ~1e-12 up to mean^2 / var ~ 1e3 and ~1e-11 at 1e4."""
    n, mean, m2 = n.double(), mean.double(), m2.double()
    nn_ = n.sum(dim)
    s = (n * mean).sum(dim)
    q = (m2 + n * mean * mean).sum(dim)
    mu = s / nn_
    var = (q / nn_ - mu * mu).clamp_min(0.0)
    return mu, var


def stats_samples(b: int, c: int, tiles: int, seed: int):
    """float64 samples (B, C, total) cut into ``tiles`` runs of ragged length 1..128 (the same cuts for every image and
    channel, as a convolution's tiles are). Channel 0 is constant (0.75), channel 1 has mean 100 and std 1.01, channel 2
    mean ~1e-17 and std 1; the rest mean in [-2, 2] and std in [0.5, 2]. Returns (samples, lengths)."""
    g = gen(seed)
    lens = torch.randint(1, 129, (tiles,), generator=g)
    total = int(lens.sum())
    mean = torch.rand(b, c, 1, generator=g, dtype=torch.float64) * 4 - 2
    std = torch.rand(b, c, 1, generator=g, dtype=torch.float64) * 1.5 + 0.5
    x = torch.randn(b, c, total, generator=g, dtype=torch.float64)
    x = x * std + mean
    x[:, 0] = 0.75

    def standardised(v):  # sample mean 0 and sample std 1 per image (a single sample stays as drawn)
        return (v - v.mean(dim=-1, keepdim=True)) / v.std(dim=-1, unbiased=False, keepdim=True) if total > 1 else v

    if c > 1:  # std 1.01: mean^2 / var = 9803, just inside the 1e4 that merge64's accuracy is stated for
        x[:, 1] = standardised(x[:, 1]) * 1.01 + 100.0
    if c > 2:
        x[:, 2] = standardised(x[:, 2])
    return x, lens


def partials64(x: torch.Tensor, lens: torch.Tensor):
    """Per-run (n, mean, M2) of ``stats_samples``' samples in float64: each (B, tiles, C)."""
    ns, means, m2s = [], [], []
    s = 0
    for l in lens.tolist():
        run = x[:, :, s:s + l]
        m = run.mean(dim=2)
        ns.append(torch.full_like(m, float(l)))
        means.append(m)
        m2s.append(((run - m[:, :, None]) ** 2).sum(dim=2))
        s += l
    return torch.stack(ns, 1), torch.stack(means, 1), torch.stack(m2s, 1)


def stats_partials_f32(b: int, c: int, n_pad: int, tiles: int, seed: int) -> torch.Tensor:
    """The kernel's input [B, tiles, n_pad, 3] fp32: partials64 rounded to fp32, NaN in the columns past C."""
    x, lens = stats_samples(b, c, tiles, seed)
    n, mean, m2 = partials64(x, lens)
    part = torch.full((b, tiles, n_pad, 3), float("nan"), dtype=torch.float32)
    part[:, :, :c, 0] = n.float()
    part[:, :, :c, 1] = mean.float()
    part[:, :, :c, 2] = m2.float()
    return part


def stats_reference(part: torch.Tensor, c: int, eps: float = EPS):
    """(a, b, max_t |mean_t|) in float64 from the fp32 partials the kernel reads: a = 1/sqrt(var + eps), b = -mean*a."""
    p = part[:, :, :c].double()
    mu, var = merge64(p[..., 0], p[..., 1], p[..., 2], dim=1)
    a = 1.0 / torch.sqrt(var + eps)
    return a, -mu * a, p[..., 1].abs().amax(dim=1)


# ------------------------------------------------------------------------------------------------- conv inputs
def conv_inputs(seed: int, b: int, cin: int, n: int, h: int, w: int, k: int):
    """fp32 input (B, cin, H, W) ~ 1.5 N(0, 1), weights (N, cin, k, k) ~ N(0, 1/(cin k^2)) and bias ~ N(0, 1): the
    distributions of tests/test_gpu_conv_s32.py's float64 cases."""
    g = gen(seed)
    x = torch.randn(b, cin, h, w, generator=g) * 1.5
    wt = torch.randn(n, cin, k, k, generator=g) / float(cin * k * k) ** 0.5
    bias = torch.randn(n, generator=g)
    return x, wt, bias


def shifted_tap(x: torch.Tensor, ky: int, kx: int) -> torch.Tensor:
    """Tap (ky, kx) of a 3x3 / stride 2 / pad 1 convolution seen alone: out[Y, X] = x[2Y + ky - 1, 2X + kx - 1], zero
    outside the image. x: (B, 2h, 2w)."""
    b, hh, ww = x.shape
    p = F.pad(x, (1, 1, 1, 1))
    return p[:, ky:ky + hh:2, kx:kx + ww:2].contiguous()


# ---------------------------------------------------------------------------------------------- whole encoder (6)
@functools.lru_cache(maxsize=None)
def encoder(norm: str) -> BasicEncoder:
    """The encoder under test on the CPU in fp32, eval mode: instance norm (RAFT's fnet, 256 outputs) or batch norm
    (cnet) with randomised running statistics and affine parameters."""
    torch.manual_seed(11 if norm == "instance" else 12)
    enc = BasicEncoder(output_dim=256, norm_fn=norm).eval()
    if norm == "batch":
        randomise_bn(enc, 1)
    for p in enc.parameters():
        p.requires_grad_(False)
    return enc


@functools.lru_cache(maxsize=None)
def encoder_case(norm: str, shape):
    """(x fp32, enc64(x) float64, e32 = max |enc32(x) - enc64(x)|) on the CPU, computed once per case and shared."""
    b, _, h, w = shape
    img0, _ = synthetic.synthetic_pair(b, h, w, seed=2)
    x = (2 * (img0 / 255.0) - 1.0).float().contiguous()
    enc = encoder(norm)
    with torch.no_grad():
        ref = copy.deepcopy(enc).double()(x.double())
        y32 = enc(x)
    e32 = float((y32.double() - ref).abs().max())
    return x, ref, e32
