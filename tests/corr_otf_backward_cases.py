"""Float64 references and deterministic inputs of the on-the-fly correlation backward tests
(csrc/corr_otf_backward.hip, ``torch.ops.oflow.corr_lookup_alt``). PyTorch on the CPU only; the window lookup, the level
sizes and the coordinate generators are tests/corr_backward_cases.py's. Not a test module.

The reference takes the fp16 tensors the prepare op returned (a = f1h, F_l = f2h[l]) as float64 leaves, builds level l as
einsum(a, F_l) -> (B*N, 1, H_l, W_l), applies ``lookup64`` and differentiates with torch autograd; the two chain steps
(1 / sqrt(C); the transpose of the iterated floor 2x2 average pools) follow in float64. The bound is the same pipeline on
|g|, |a|, |F_l| (every lookup weight is non-negative): the operand magnitude an fp32 evaluation's rounding error scales
with, zero exactly where no window term lands.

GPU tolerance: K * 2^-24 * bound + 1e-30 per element. K = 4 x the worst |err| / (2^-24 * bound) of the same composition
run in fp32 on the CPU under autograd (level matmuls, lookup, chain steps) at the fp16-valued inputs of ``GAUSS_CASES``,
against float64: measured on that reference composition (tests/test_corr_otf_backward_host.py), never on the kernel. The
factor 4 is the project's margin for another summation order (MFMA chains, atomic arrival order).
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import torch
import torch.nn.functional as F

import corr_backward_cases as cc

EPS24 = 2.0**-24
# worst |err| / (2^-24 * bound) of the fp32 CPU composition over GAUSS_CASES: grad_fmap1 / grad_fmap2 (host test)
CALIBRATED_RATIO_G1 = 3.13  # measured 3.125 -> K = 12.52
CALIBRATED_RATIO_G2 = 3.15  # measured 3.149 -> K = 12.60
K_G1 = 4.0 * CALIBRATED_RATIO_G1
K_G2 = 4.0 * CALIBRATED_RATIO_G2

# (radius, (H0, W0), levels, C, coordinate kind): B = 2 throughout.
#   mixed  : cc.mixed_coords -- windows inside / straddling / outside, integers and negative fractions; scattered over
#            the level, so level 0's box exceeds kTMax (per-query passes) while the higher levels fit
#   smooth : grid + N(0, 1.5^2): the box pass at every level whose box fits (level 0 for the narrower windows)
#   still  : grid + N(0, 0.25^2): level 0 takes the box pass at radius 4 too
GAUSS_CASES = (
    [(r, (17, 37), 4, 64, "mixed") for r in range(5)]
    + [(r, (17, 37), 4, 64, "smooth") for r in range(5)]
    + [(4, (17, 37), 4, 64, "still")]
    + [(4, (5, 13), 2, 32, "mixed"), (2, (5, 13), 2, 32, "smooth")]  # ragged segments in both directions
    + [(4, (9, 35), 3, 96, "mixed"), (3, (9, 35), 3, 96, "smooth")]  # sqrt(C) no power of two, 3 segments per row
)
CASE_IDS = [f"r{r}-{h}x{w}-L{l}-C{c}-{kind}" for r, (h, w), l, c, kind in GAUSS_CASES]
BATCH = 2
# the exact (dyadic) case and the stray-coordinate case
DYADIC = (4, (17, 37), 4, 64)
SPECIALS = (4, (17, 37), 4, 64)


def case_seed(case) -> int:
    r, (h, w), levels, c, kind = case
    return 10000 + 1000 * r + 10 * h + w + 7 * levels + c + {"mixed": 0, "smooth": 300000, "still": 600000}[kind]


def grid_coords(b: int, h: int, w: int) -> torch.Tensor:
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return torch.stack((xs, ys), dim=0).float()[None].repeat(b, 1, 1, 1)


def case_inputs(case):
    """(fmap1, fmap2, coords, grad_out) of one Gaussian case, fp32 on the CPU. In the last pair the output gradient is
    kept only at level 0 and only for every 61st query, so that elements no window term reaches (bound 0) occur in
    both gradients."""
    r, (h, w), levels, c, kind = case
    seed, k = case_seed(case), 2 * r + 1
    f1, f2 = cc.gaussian(seed + 1, (BATCH, c, h, w)), cc.gaussian(seed + 2, (BATCH, c, h, w))
    if kind == "mixed":
        coords = cc.mixed_coords(seed % 9973, (BATCH, 2, h, w), r, h, w)
    else:
        coords = grid_coords(BATCH, h, w) + (1.5 if kind == "smooth" else 0.25) * cc.gaussian(seed + 3, (BATCH, 2, h, w))
    g = cc.gaussian(seed + 4, (BATCH, levels * k * k, h, w))
    g[-1, k * k:] = 0
    keep = (torch.arange(h * w) % 61 == 0).reshape(1, h, w)
    g[-1, : k * k] *= keep
    return f1, f2, coords, g


def dyadic_inputs():
    """Integer feature maps (fmap1 in [-4, 4], fmap2 in [-2, 2]), C = 64 (1 / sqrt(C) = 2^-3), half-pixel coordinates and
    an output gradient in {-1, 0, 1}: fmap1 / 8 and every pooled level of fmap2 are exact in fp16, level-l weights are
    multiples of 4^-(l+1), so every product and partial sum of either gradient is a multiple of 2^-17 (level 3:
    2^-8 weights x 2^-6 pooled features x 2^-3), exact in fp32 while it stays below 2^7."""
    r, (h, w), levels, c = DYADIC
    f1 = cc.integers(71, (BATCH, c, h, w), 4)
    f2 = cc.integers(72, (BATCH, c, h, w), 2)
    coords = cc.lattice_coords(73, (BATCH, 2, h, w), r, h, w, 2)
    g = cc.integers(74, (BATCH, levels * (2 * r + 1) ** 2, h, w), 1)
    return f1, f2, coords, g


DYADIC_QUANTUM_BITS = 17  # m: every partial sum is a multiple of 2^-m and must stay below 2^(24-m)


def prepare_emulated(fmap1: torch.Tensor, fmap2: torch.Tensor, levels: int):
    """What corr_otf_prepare stores, on the CPU: f1h = fp16(fmap1 * fp32(1 / sqrt(C))) as (B, H, W, C) and f2h[l] =
    fp16 of the fp32 iterated floor 2x2 average pool of fmap2 as (B, H_l, W_l, C)."""
    c = fmap1.shape[1]
    scale = torch.tensor(1.0 / math.sqrt(c), dtype=torch.float32)
    f1h = (fmap1.float() * scale).permute(0, 2, 3, 1).contiguous().half()
    f2h, cur = [], fmap2.float()
    for l in range(levels):
        if l:
            cur = F.avg_pool2d(cur, 2, stride=2)
        f2h.append(cur.permute(0, 2, 3, 1).contiguous().half())
    return f1h, f2h


# ------------------------------------------------------------------------------------------------ the lookup, any dtype
def lookup_like(levels: Sequence[torch.Tensor], coords: torch.Tensor, radius: int) -> torch.Tensor:
    """``cc.lookup64`` in the levels' own dtype: the window origin and the fractions come from float64 (exact in fp32
    too: c / 2^l, floor and their difference are exact), the weights and the sums are formed in the levels' dtype."""
    dt = levels[0].dtype
    if dt == torch.float64:
        return cc.lookup64(levels, coords, radius)
    r = int(radius)
    k, pk = 2 * r + 1, 2 * r + 2
    b, _, h, w = coords.shape
    q = b * h * w
    c64 = coords.detach().to(torch.float64)
    cx0, cy0 = c64[:, 0].reshape(q), c64[:, 1].reshape(q)
    off = torch.arange(pk, dtype=torch.int64)
    outs = []
    for l, lvl in enumerate(levels):
        hl, wl = (int(v) for v in lvl.shape[-2:])
        p = lvl.reshape(q, hl * wl)
        cx, cy = cx0 / float(2**l), cy0 / float(2**l)
        ok = torch.isfinite(cx) & torch.isfinite(cy) & (cx.abs() < cc.COORD_LIMIT) & (cy.abs() < cc.COORD_LIMIT)
        cx, cy = torch.where(ok, cx, torch.zeros_like(cx)), torch.where(ok, cy, torch.zeros_like(cy))
        x0, y0 = torch.floor(cx), torch.floor(cy)
        wx, wy = (cx - x0).to(dt)[:, None, None], (cy - y0).to(dt)[:, None, None]
        xs = (x0.to(torch.int64) - r)[:, None] + off[None, :]
        ys = (y0.to(torch.int64) - r)[:, None] + off[None, :]
        inx, iny = (xs >= 0) & (xs < wl), (ys >= 0) & (ys < hl)
        idx = ys.clamp(0, hl - 1)[:, :, None] * wl + xs.clamp(0, wl - 1)[:, None, :]
        mask = (iny[:, :, None] & inx[:, None, :] & ok[:, None, None]).to(dt)
        patch = p.gather(1, idx.reshape(q, pk * pk)).reshape(q, pk, pk) * mask
        s = ((1 - wy) * (1 - wx) * patch[:, :-1, :-1] + (1 - wy) * wx * patch[:, :-1, 1:]
             + wy * (1 - wx) * patch[:, 1:, :-1] + wy * wx * patch[:, 1:, 1:])
        outs.append(s.transpose(1, 2).reshape(q, k * k))
    return torch.cat(outs, dim=1).reshape(b, h, w, len(outs) * k * k).permute(0, 3, 1, 2).contiguous()


# -------------------------------------------------------------------------------------------------------- references
def fold_levels(gfs: Sequence[torch.Tensor]) -> torch.Tensor:
    """sum_l gF_l[b, y >> l, x >> l, c] / 4^l where (y >> l, x >> l) is inside level l, as (B, C, H, W): the transpose
    of the iterated floor 2x2 average pools (oflow_corr_pyramid_grad_combine_f32's rule), in the inputs' dtype."""
    b, h0, w0, c = gfs[0].shape
    acc = gfs[0].clone()
    y, x = torch.arange(h0), torch.arange(w0)
    for l in range(1, len(gfs)):
        hl, wl = gfs[l].shape[1:3]
        yl, xl = y >> l, x >> l
        inside = ((yl < hl)[:, None] & (xl < wl)[None, :]).to(acc.dtype)[None, :, :, None]
        acc = acc + gfs[l][:, yl.clamp(max=hl - 1)][:, :, xl.clamp(max=wl - 1)] * inside * (0.25**l)
    return acc.permute(0, 3, 1, 2).contiguous()


def _pipeline(a: torch.Tensor, fs: Sequence[torch.Tensor], coords: torch.Tensor, g: torch.Tensor, radius: int):
    """(grad_fmap1, grad_fmap2) as (B, C, H, W) in the dtype of ``a``: autograd through einsum + lookup, then the two
    chain steps."""
    b, h, w, c = a.shape
    a = a.detach().clone().requires_grad_()
    fs = [f.detach().clone().requires_grad_() for f in fs]
    levels = [torch.einsum("bqc,btc->bqt", a.reshape(b, h * w, c), f.reshape(b, -1, c)).reshape(b * h * w, 1, f.shape[1], f.shape[2])
              for f in fs]
    out = lookup_like(levels, coords, radius)
    ga, *gfs = torch.autograd.grad(out, [a] + fs, g.to(a.dtype))
    scale = torch.tensor(1.0 / math.sqrt(c), dtype=a.dtype)
    return ga.permute(0, 3, 1, 2).contiguous() * scale, fold_levels(gfs)


def reference64(f1h: torch.Tensor, f2h: Sequence[torch.Tensor], coords: torch.Tensor, g: torch.Tensor, radius: int):
    """Float64 (grad_fmap1, grad_fmap2) of the lookup at the stored fp16 values."""
    return _pipeline(f1h.double(), [f.double() for f in f2h], coords, g.double(), radius)


def bound64(f1h: torch.Tensor, f2h: Sequence[torch.Tensor], coords: torch.Tensor, g: torch.Tensor, radius: int):
    """The same pipeline on |g|, |a|, |F_l|."""
    return _pipeline(f1h.double().abs(), [f.double().abs() for f in f2h], coords, g.double().abs(), radius)


def composition32(f1h: torch.Tensor, f2h: Sequence[torch.Tensor], coords: torch.Tensor, g: torch.Tensor, radius: int):
    """The composition in fp32 on the CPU (what K is calibrated on)."""
    return _pipeline(f1h.float(), [f.float() for f in f2h], coords, g.float(), radius)


def dense_composition64(fmap1: torch.Tensor, fmap2: torch.Tensor, coords: torch.Tensor, g: torch.Tensor, levels: int,
                        radius: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Float64 autograd of the reference project's own definition: matmul / sqrt(C), avg_pool2d of the volume, window
    lookup (cc.corr_levels64 + cc.lookup64) -> (grad_fmap1, grad_fmap2)."""
    a1, a2 = fmap1.double().requires_grad_(), fmap2.double().requires_grad_()
    out = cc.lookup64(cc.corr_levels64(a1, a2, levels), coords, radius)
    g1, g2 = torch.autograd.grad(out, [a1, a2], g.double())
    return g1, g2


def tolerances(b1: torch.Tensor, b2: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    return K_G1 * EPS24 * b1 + 1e-30, K_G2 * EPS24 * b2 + 1e-30


def level_shapes(h: int, w: int, levels: int) -> List[Tuple[int, int]]:
    return cc.level_dims(h, w, levels)
