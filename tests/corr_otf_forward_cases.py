"""Float64 references, deterministic inputs and constants of the on-the-fly correlation forward tests
(csrc/corr_otf.hip: ``torch.ops.oflow.corr_otf_prepare`` and ``torch.ops.oflow.corr_lookup_otf``). NumPy / PyTorch on
the CPU only; the Gaussian cases, the dyadic inputs and the coordinate generators are tests/corr_otf_backward_cases.py's
and tests/corr_backward_cases.py's. Not a test module.

Reference: the fp16 tensors the prepare step stored are the operands. ``forward64`` builds level l as
einsum(f1h, f2h[l]) in float64 and applies the window lookup with the fractions as the kernel's contract forms them:
cx = coord * 2^-l (exact), wx = fp32(cx - floor(cx)) (one fp32 rounding: a negative coordinate just below an integer has a
fraction fp32 cannot hold, and that rounding is the fp32 definition of the operation, not kernel error), ex = 1 - wx and
every product and sum from there in float64. ``bound64`` is the same pipeline on |f1h|, |f2h[l]| (every weight is
non-negative): the operand magnitude an fp32 evaluation's rounding error scales with, zero exactly where every tap of an
output lies outside the level.

GPU tolerance: K_FWD * 2^-24 * bound + 1e-30 per element, K_FWD = 4 x the worst |err| / (2^-24 * bound) of the same
composition run in fp32 on the CPU (``composition32``) against ``forward64`` over ``CASES`` at the ``prepare_exact``
tensors: measured on that reference composition (tests/test_corr_otf_forward_host.py), never on the kernel. The factor
4 is the project's margin for another summation order (the MFMA's k-chain).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import corr_backward_cases as cc
import corr_otf_backward_cases as oc

EPS24 = oc.EPS24
# worst |err| / (2^-24 * bound) of the fp32 CPU composition over CASES (host test)
CALIBRATED_RATIO_FWD = 4.72  # measured 4.714 (r4-17x37-L4-C64-still; 4.495 with another CPU's BLAS, r4 mixed) -> K = 18.88
K_FWD = 4.0 * CALIBRATED_RATIO_FWD

# (radius, (H0, W0), levels, C, coordinate kind, B). The first block is oc.GAUSS_CASES with their own inputs (B = 2);
# the rest are the forward's own:
#   C = 256 (eight 32-channel K-steps of the MFMA chain), B = 3, a last level of exactly 2 x 2 (the smallest the lookup
#   takes), W = 16 / 17 (exactly one 16-query segment / one segment plus one column), H = 2 / 3 (one segment row / one
#   plus a ragged one), and `away`: two segments in three sent beyond every level by more than the window (the zero fill)
CASES: List[tuple] = (
    [case + (oc.BATCH,) for case in oc.GAUSS_CASES]
    + [(4, (17, 37), 4, 256, "smooth", 2), (4, (17, 37), 4, 256, "mixed", 2)]
    + [(3, (5, 13), 2, 32, "mixed", 3)]
    + [(3, (17, 19), 4, 32, "smooth", 2)]
    + [(4, (6, 16), 2, 32, "smooth", 2), (2, (6, 16), 2, 32, "mixed", 2)]
    + [(4, (6, 17), 2, 32, "smooth", 2), (2, (6, 17), 2, 32, "mixed", 2)]
    + [(4, (2, 21), 1, 32, "smooth", 2), (4, (3, 21), 1, 32, "mixed", 2)]
    + [(4, (17, 37), 4, 64, "away", 2)]
)


def case_id(case) -> str:
    r, (h, w), levels, c, kind, b = case
    return f"r{r}-{h}x{w}-L{levels}-C{c}-{kind}" + ("" if b == oc.BATCH else f"-B{b}")


CASE_IDS = [case_id(case) for case in CASES]
DYADIC = oc.DYADIC
DYADIC_QUANTUM_BITS = oc.DYADIC_QUANTUM_BITS
# the grid of the neighbour-independence and kTMax-edge tests: levels 0 and 1 both hold more than T_MAX targets
PATH_GRID = dict(b=1, h=40, w=48, c=32, levels=3, radius=4)

# the kernel's segment rule
SEG_ROWS, SEG_COLS, T_MAX = 2, 16, 384
OUTSIDE, BOX, PER_QUERY = 0, 1, 2


# ------------------------------------------------------------------------------------------------------------ inputs
def _kind_coords(kind: str, seed: int, b: int, h: int, w: int, r: int) -> torch.Tensor:
    if kind == "mixed":
        return cc.mixed_coords(seed % 9973, (b, 2, h, w), r, h, w)
    sigma = {"smooth": 1.5, "still": 0.25, "away": 1.5}[kind]
    co = oc.grid_coords(b, h, w) + sigma * cc.gaussian(seed + 3, (b, 2, h, w))
    if kind == "away":
        # segment s: s % 3 == 1 -> x + 1000 (right of every level), s % 3 == 2 -> y - 16 (r + 3) (above every level of
        # up to 4: -16 (r + 3) / 8 + r + 1 < 0); the others stay
        segx = -(-w // SEG_COLS)
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        seg = (ys // SEG_ROWS) * segx + xs // SEG_COLS
        co[:, 0] += 1000.0 * (seg % 3 == 1)
        co[:, 1] -= (16.0 * (r + 3) + h) * (seg % 3 == 2)
    return co


def inputs(case) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(fmap1, fmap2, coords) of one case, fp32 on the CPU."""
    r, (h, w), levels, c, kind, b = case
    if case[:5] in oc.GAUSS_CASES and b == oc.BATCH:
        return oc.case_inputs(case[:5])[:3]
    seed = 500000 + 1000 * r + 10 * h + w + 7 * levels + c + 100003 * b + {"mixed": 0, "smooth": 30000, "still": 60000,
                                                                            "away": 90000}[kind]
    f1, f2 = cc.gaussian(seed + 1, (b, c, h, w)), cc.gaussian(seed + 2, (b, c, h, w))
    return f1, f2, _kind_coords(kind, seed, b, h, w, r)


def path_grid_features() -> Tuple[torch.Tensor, torch.Tensor]:
    g = PATH_GRID
    return cc.gaussian(811, (g["b"], g["c"], g["h"], g["w"])), cc.gaussian(812, (g["b"], g["c"], g["h"], g["w"]))


def still_coords() -> torch.Tensor:
    """Run A of the neighbour-independence test: grid + N(0, 0.2^2), every segment's box fits at every level."""
    g = PATH_GRID
    return oc.grid_coords(g["b"], g["h"], g["w"]) + 0.2 * cc.gaussian(813, (g["b"], 2, g["h"], g["w"]))


def scattered_coords() -> Tuple[torch.Tensor, torch.Tensor]:
    """Run B: ``still_coords`` with two queries of every segment moved to opposite corners of the level, still inside it
    (one moved query is not enough at level 1: 20 x 24 = 480 targets, and the box of a central segment plus one corner
    is 21 x 16 = 336 <= 384). Their windows then span the whole level: no segment fits at levels 0 and 1 (1920 and 480
    targets). Returns (coords, the (H, W) mask of the moved queries)."""
    g = PATH_GRID
    co = still_coords()
    moved = torch.zeros(g["h"], g["w"], dtype=torch.bool)
    for y0 in range(0, g["h"], SEG_ROWS):
        for x0 in range(0, g["w"], SEG_COLS):
            s = (y0 // SEG_ROWS) * 3 + x0 // SEG_COLS
            qa, qb = (y0, x0 + (5 * s) % SEG_COLS), (y0 + 1, x0 + (7 * s + 3) % SEG_COLS)
            co[:, 0, qa[0], qa[1]], co[:, 1, qa[0], qa[1]] = 0.5, 0.25
            co[:, 0, qb[0], qb[1]], co[:, 1, qb[0], qb[1]] = g["w"] - 1.5, g["h"] - 1.25
            moved[qa], moved[qb] = True, True
    return co, moved


KTMAX_SEGMENT = (8, 1)  # (segment row, segment column) of PATH_GRID: queries rows 16-17, columns 16-31, interior


def ktmax_coords(shift_cols: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Integer coordinates (level 0 is an exact gather) with, in the interior segment ``KTMAX_SEGMENT``, the last query of
    the second row shifted by +``shift_cols`` columns and the first query of that row by +1 row: at radius 4 the
    segment's level-0 box is 12 x (25 + shift_cols): 12 x 32 = 384 = T_MAX at +7, 12 x 33 = 396 at +8. Returns (coords,
    the (H, W) mask of the two shifted queries)."""
    g = PATH_GRID
    co = oc.grid_coords(g["b"], g["h"], g["w"])
    y, x = KTMAX_SEGMENT[0] * SEG_ROWS + 1, KTMAX_SEGMENT[1] * SEG_COLS
    co[:, 1, y, x] += 1.0
    co[:, 0, y, x + SEG_COLS - 1] += float(shift_cols)
    touched = torch.zeros(g["h"], g["w"], dtype=torch.bool)
    touched[y, x], touched[y, x + SEG_COLS - 1] = True, True
    return co, touched


# --------------------------------------------------------------------------------------------- the prepare step, exact
def prepare_scale(c: int) -> np.float32:
    """The kernel's host code ``1.0f / sqrtf((float)C)``: an fp32 square root and an fp32 division (one ulp away from
    fp32(1 / sqrt(C)) computed in double at C = 96, 288, 384, 448 within C <= 512)."""
    return np.float32(1.0) / np.sqrt(np.float32(c))


def prepare_exact(fmap1: torch.Tensor, fmap2: torch.Tensor, levels: int):
    """What corr_otf_prepare stores, bit for bit: f1h = fp16_rne(fp32(fmap1 * s)) as (B, H, W, C) with s =
    ``prepare_scale(C)``; f2h[l] = fp16_rne of the fp32 iterated floor 2x2 average pool of fmap2 in ATen's summation order
    (F.avg_pool2d on the CPU) as (B, H_l, W_l, C)."""
    s = torch.tensor(float(prepare_scale(fmap1.shape[1])), dtype=torch.float32)
    assert float(s) == float(prepare_scale(fmap1.shape[1]))
    f1h = (fmap1.float() * s).permute(0, 2, 3, 1).contiguous().half()
    f2h, cur = [], fmap2.float()
    for l in range(levels):
        if l:
            cur = F.avg_pool2d(cur, 2, stride=2)
        f2h.append(cur.permute(0, 2, 3, 1).contiguous().half())
    return f1h, f2h


# (C, (H, W), B, levels) of the bit-for-bit prepare test: C = 32 / 96 / 160 are ragged in to_nhwc_f16_kernel's 64-channel
# block, sqrt(96) and sqrt(160) are no powers of two; odd sizes at several levels (the floor drops a row and a column);
# no H * W is a multiple of 64 (ragged 64-pixel block)
PREPARE_CASES = [
    (32, (17, 37), 1, 4), (96, (17, 37), 3, 4), (160, (17, 37), 1, 3), (256, (17, 37), 1, 4),
    (96, (5, 13), 3, 2), (256, (5, 13), 1, 2), (160, (9, 35), 3, 3), (32, (9, 35), 1, 1),
    (32, (2, 2), 3, 1), (160, (2, 2), 1, 2), (96, (2, 2), 1, 1), (256, (2, 2), 3, 2),
]


def prepare_inputs(index: int) -> Tuple[torch.Tensor, torch.Tensor]:
    c, (h, w), b, _ = PREPARE_CASES[index]
    return cc.gaussian(900 + 2 * index, (b, c, h, w)), cc.gaussian(901 + 2 * index, (b, c, h, w))


def planted_values() -> List[float]:
    """fp32 values whose fp16 rounding is an edge: -0.0, subnormals (2^-24 is the smallest; 2^-25 ties to 0, 3 * 2^-25
    ties to 2^-23, just above / below 2^-25), the largest subnormal and smallest normal, round-to-even ties at 1 and at
    2048, +-65504 (the largest finite), the largest fp32 below the tie 65520, and +-65520 itself (rounds to inf)."""
    t = 2.0**-11
    vals = [-0.0, 2.0**-24, -(2.0**-24), 2.0**-25, 3 * 2.0**-25, -3 * 2.0**-25, 2.0**-25 * (1 + 2.0**-20),
            2.0**-25 * (1 - 2.0**-20), 1.5 * 2.0**-15, 1023 * 2.0**-24, 1023.5 * 2.0**-24, 2.0**-14, 5.25 * 2.0**-24,
            1 + t, 1 + 3 * t, -(1 + t), -(1 + 3 * t), 1 + t + 2.0**-23, 1 + t - 2.0**-23, 2049.0, 2051.0,
            65504.0, -65504.0, 65519.996, 65520.0, -65520.0]
    return [float(np.float32(v)) for v in vals]


PLANTED = (64, (5, 13), 3, 3)  # (C, (H, W), B, levels); C = 64: s = 2^-3 exactly, so fmap1 holds 8 x the planted values


def planted_inputs() -> Tuple[torch.Tensor, torch.Tensor]:
    """Gaussian maps of the ``PLANTED`` shape with ``planted_values`` written along channel 3 (fmap2, level 0) and 8 x
    them along channel 5 of fmap1, and 2x2 blocks of fmap2 whose fp32 average is an exact fp16 tie although no element
    is fp16-representable (pooled levels 1 and 2: rounding before the pool would give another value)."""
    c, (h, w), b, _ = PLANTED
    f1, f2 = cc.gaussian(990, (b, c, h, w)), cc.gaussian(991, (b, c, h, w))
    vals = torch.tensor(planted_values(), dtype=torch.float32)
    n = vals.numel()
    assert n <= h * w
    f2[0, 3].view(-1)[:n] = vals
    f1[0, 5].view(-1)[:n] = vals * 8.0
    t = 2.0**-11
    for ch, tie, e in ((7, 1 + t, 2.0**-13), (8, 1 + 3 * t, -(2.0**-13)), (9, -(2 + 2 * t), -(2.0**-12))):
        # level 1 pixel (0, 0): three values a quarter of an fp16 step to one side of the tie and one three quarters to
        # the other; every partial sum is exact in fp32 and the sum is 4 x tie. Rounded first, three of them move away
        # from the side the tie rounds to
        block = torch.tensor([[tie + e, tie + e], [tie + e, tie - 3 * e]], dtype=torch.float32)
        assert bool((block.half().float() != block).all()) and float(block.double().sum()) == 4 * tie
        f2[1, ch, :2, :2] = block
        # level 2 pixel (0, 0) = the average of 16 values: all four level-1 pixels equal the tie
        f2[2, ch, :4, :4] = block.repeat(2, 2)
    return f1, f2


# ------------------------------------------------------------------------------------------------- the forward, any dtype
def window_lookup(levels: Sequence[torch.Tensor], coords: torch.Tensor, radius: int,
                  perturb: Optional[Dict] = None) -> torch.Tensor:
    """``cc.lookup64`` with the fractions as the kernel's contract forms them: per level cx = coord * 2^-l (exact), wx =
    fp32(cx - floor(cx)), then ex = 1 - wx, the four weights and the sums in the levels' own dtype (float64: the
    reference; float32: the composition K is calibrated on). ``levels[l]`` is (B*H*W, H_l * W_l)-viewable; NaN / inf /
    |c| >= 2^22 in either coordinate gives an all-zero window.

    ``perturb`` (the host test's sensitivity check only) breaks the lookup the way a kernel bug would:
    {"weight": s} scales the (y + 1, x + 1) tap's weight by s; {"drop_corner": l} drops the (y + 1, x + 1) tap where it
    lands on the last row and column of level l."""
    perturb = perturb or {}
    dt = levels[0].dtype
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
        wx, wy = (cx - x0).float().to(dt)[:, None, None], (cy - y0).float().to(dt)[:, None, None]
        ex, ey = 1 - wx, 1 - wy
        xs = (x0.to(torch.int64) - r)[:, None] + off[None, :]
        ys = (y0.to(torch.int64) - r)[:, None] + off[None, :]
        inx, iny = (xs >= 0) & (xs < wl), (ys >= 0) & (ys < hl)
        idx = ys.clamp(0, hl - 1)[:, :, None] * wl + xs.clamp(0, wl - 1)[:, None, :]  # (q, rows, columns)
        mask = (iny[:, :, None] & inx[:, None, :] & ok[:, None, None]).to(dt)
        patch = p.gather(1, idx.reshape(q, pk * pk)).reshape(q, pk, pk) * mask
        p11 = patch[:, 1:, 1:]
        if perturb.get("drop_corner") == l:
            p11 = p11 * (~((ys[:, 1:, None] == hl - 1) & (xs[:, None, 1:] == wl - 1))).to(dt)
        w11 = wy * wx * torch.tensor(perturb.get("weight", 1.0), dtype=dt)
        s = ey * ex * patch[:, :-1, :-1] + ey * wx * patch[:, :-1, 1:] + wy * ex * patch[:, 1:, :-1] + w11 * p11
        outs.append(s.transpose(1, 2).reshape(q, k * k))  # channel i (column) * K + j (row)
    return torch.cat(outs, dim=1).reshape(b, h, w, len(outs) * k * k).permute(0, 3, 1, 2).contiguous()


def _forward(a: torch.Tensor, fs: Sequence[torch.Tensor], coords: torch.Tensor, radius: int,
             perturb: Optional[Dict] = None) -> torch.Tensor:
    b, h, w, c = a.shape
    levels = [torch.einsum("bqc,btc->bqt", a.reshape(b, h * w, c), f.reshape(b, -1, c)).reshape(b * h * w, f.shape[1], f.shape[2])
              for f in fs]
    if perturb and "shift_target" in perturb:
        # the last target of level l's last partial 16-column N-tile reads its neighbour's features
        l = perturb["shift_target"]
        hl, wl = levels[l].shape[-2:]
        assert (hl * wl) % 16 != 0
        flat = levels[l].reshape(b * h * w, hl * wl).clone()
        flat[:, -1] = flat[:, -2]
        levels[l] = flat.reshape(b * h * w, hl, wl)
    return window_lookup(levels, coords, radius, perturb)


def forward64(f1h: torch.Tensor, f2h: Sequence[torch.Tensor], coords: torch.Tensor, radius: int) -> torch.Tensor:
    """Float64 output (B, L*(2r+1)^2, H, W) of the lookup at the stored fp16 values."""
    return _forward(f1h.double(), [f.double() for f in f2h], coords, radius)


def bound64(f1h: torch.Tensor, f2h: Sequence[torch.Tensor], coords: torch.Tensor, radius: int) -> torch.Tensor:
    """The same pipeline on |f1h|, |f2h[l]|."""
    return _forward(f1h.double().abs(), [f.double().abs() for f in f2h], coords, radius)


def composition32(f1h: torch.Tensor, f2h: Sequence[torch.Tensor], coords: torch.Tensor, radius: int,
                  perturb: Optional[Dict] = None) -> torch.Tensor:
    """The composition in fp32 on the CPU (what K_FWD is calibrated on)."""
    return _forward(f1h.float(), [f.float() for f in f2h], coords, radius, perturb)


def dense_definition64(fmap1: torch.Tensor, fmap2: torch.Tensor, coords: torch.Tensor, levels: int,
                       radius: int) -> torch.Tensor:
    """The reference project's own definition in float64: matmul / sqrt(C), avg_pool2d of the volume, window lookup."""
    return cc.lookup64(cc.corr_levels64(fmap1.double(), fmap2.double(), levels), coords, radius)


def tolerance(bound: torch.Tensor) -> torch.Tensor:
    return K_FWD * EPS24 * bound + 1e-30


# ------------------------------------------------------------------------------------------------------- path census
def census(coords: torch.Tensor, radius: int, dims: Sequence[Tuple[int, int]]) -> List[Dict[str, np.ndarray]]:
    """The kernel's segment rule restated on the host. Queries are grouped into segments of SEG_ROWS x SEG_COLS; at level l
    a query's window (origin floor(coord * 2^-l) - r, side 2r + 2; none for NaN / inf / |c| >= 2^22) is included iff it
    overlaps the level; the box of the included windows is clipped to the level and fits iff its area is at most T_MAX.
    Per level: ``kind`` (B, segy, segx) in {OUTSIDE, BOX, PER_QUERY} and ``area`` (the clipped box's targets, 0 for
    OUTSIDE). A BOX segment runs nT = ceil(area / 16) N-tiles and its last LDS column is area - 1."""
    co = coords.detach().numpy().astype(np.float32)
    b, _, h, w = co.shape
    r, pk = int(radius), 2 * int(radius) + 2
    segy, segx = -(-h // SEG_ROWS), -(-w // SEG_COLS)
    far = np.int64(1) << 40
    out = []
    for l, (hl, wl) in enumerate(dims):
        inv = np.float32(1.0) / np.float32(1 << l)
        with np.errstate(invalid="ignore", over="ignore"):
            cx, cy = co[:, 0] * inv, co[:, 1] * inv  # fp32, as the kernel
            ok = (np.abs(cx) < np.float32(cc.COORD_LIMIT)) & (np.abs(cy) < np.float32(cc.COORD_LIMIT))
        xs = np.floor(np.where(ok, cx, np.float32(0))).astype(np.int64) - r
        ys = np.floor(np.where(ok, cy, np.float32(0))).astype(np.int64) - r
        inc = ok & (ys + pk > 0) & (ys < hl) & (xs + pk > 0) & (xs < wl)

        def seg(v, fill):
            full = np.full((b, segy * SEG_ROWS, segx * SEG_COLS), fill, dtype=v.dtype)
            full[:, :h, :w] = v
            return full.reshape(b, segy, SEG_ROWS, segx, SEG_COLS)

        any_ = seg(inc, False).any(axis=(2, 4))
        by0 = np.maximum(seg(np.where(inc, ys, far), far).min(axis=(2, 4)), 0)
        bx0 = np.maximum(seg(np.where(inc, xs, far), far).min(axis=(2, 4)), 0)
        by1 = np.minimum(seg(np.where(inc, ys + pk - 1, -far), -far).max(axis=(2, 4)), hl - 1)
        bx1 = np.minimum(seg(np.where(inc, xs + pk - 1, -far), -far).max(axis=(2, 4)), wl - 1)
        area = np.where(any_, (by1 - by0 + 1) * (bx1 - bx0 + 1), 0)
        assert bool((area[any_] > 0).all())
        kind = np.where(~any_, OUTSIDE, np.where(area <= T_MAX, BOX, PER_QUERY))
        out.append({"kind": kind, "area": area, "rows": np.where(any_, by1 - by0 + 1, 0),
                    "cols": np.where(any_, bx1 - bx0 + 1, 0)})
    return out


def census_counts(cen: Sequence[Dict[str, np.ndarray]]) -> List[Tuple[int, int, int]]:
    """Per level (all-outside, box pass, per-query) segment counts."""
    return [tuple(int((c["kind"] == k).sum()) for k in (OUTSIDE, BOX, PER_QUERY)) for c in cen]
