"""Float64 brute-force reference and the case table of the forward_interpolate tests (csrc/forward_interpolate.hip,
model.utils.forward_interpolate). NumPy only; every input comes from a seeded generator or is written out, so every
machine rebuilds it bit for bit. Not a test module.

The reference states the contract of include/oflow.h literally. Per image, in float64: source s = y*W + x lands at
(x1, y1) = (x + dx[s], y + dy[s]) and is landed iff 0 < x1 < W and 0 < y1 < H; query (qx, qy) takes the fp32 flow of the
landed source with the least (qx - x1)**2 + (qy - y1)**2, the LOWEST s among equals (np.argmin returns the first
minimum of the full distance matrix, whose columns are the sources in index order); zeros when nothing landed.

The comparison with an implementation is exact (np.array_equal). That is legitimate where the implementation's
distances are the reference's bit for bit (same float64 operations, each rounded once: then equal distances tie in both
and both take the lowest index), and it does not even lean on that where no two candidates come close: for every random
case the module asserts, when it builds the case's reference, that the best and second-best squared distance of every
query differ by >= MIN_GAP = 1e-9, seven orders above float64 rounding of distances of this size. The tie and the
constant cases are dyadic: their distances are exact in any evaluation order, and their ties are real.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Tuple

import numpy as np

MIN_GAP = 1e-9


class Case(NamedTuple):
    name: str
    flow: np.ndarray  # (B, 2, H, W) float32
    random: bool  # the gap assertion applies


def interpolate64(flow: np.ndarray) -> Tuple[np.ndarray, float]:
    """(forward_interpolate of one (2, H, W) fp32 image by brute force in float64, the smallest gap between the best and
    the second-best squared distance over its queries; inf with fewer than two landed sources)."""
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[0] == 2
    _, h, w = flow.shape
    n = h * w
    s = np.arange(n)
    gx, gy = (s % w).astype(np.float64), (s // w).astype(np.float64)
    f = flow.reshape(2, n)
    with np.errstate(invalid="ignore"):
        x1, y1 = gx + f[0].astype(np.float64), gy + f[1].astype(np.float64)
        landed = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)  # all false for NaN, one false for +-inf
    out = np.zeros((2, n), np.float32)
    if not landed.any():
        return out.reshape(2, h, w), np.inf
    x1, y1 = np.where(landed, x1, 0.0), np.where(landed, y1, 0.0)
    gap = np.inf
    rows = max(1, (1 << 22) // n)  # queries per slab of the distance matrix (<= 32 MiB)
    for q0 in range(0, n, rows):
        dx = gx[q0:q0 + rows, None] - x1[None, :]
        dy = gy[q0:q0 + rows, None] - y1[None, :]
        d2 = dx * dx + dy * dy
        d2[:, ~landed] = np.inf
        best = d2.argmin(axis=1)  # first minimum = lowest source index
        out[:, q0:q0 + rows] = f[:, best]
        if n > 1:
            two = np.partition(d2, 1, axis=1)[:, :2]
            with np.errstate(invalid="ignore"):
                g = two[:, 1] - two[:, 0]  # (inf - inf with one landed source: no second candidate)
            gap = min(gap, float(np.nanmin(np.where(np.isnan(g), np.inf, g))))
    return out.reshape(2, h, w), gap


def gaussian(h: int, w: int, sigma: float, seed: int) -> np.ndarray:
    return (np.random.default_rng(seed).standard_normal((2, h, w)) * sigma).astype(np.float32)


# (H, W, sigma, seed). Small to Sintel-sized grids, mild to wild flows (17x33 lands 23 of 561 sources). 33x65 = 2145 sources: more
# than one 2048-entry LDS tile, and no multiple of the 32 queries of a workgroup.
RANDOM = [(5, 7, 1.5, 0), (9, 13, 3.0, 1), (11, 17, 3.0, 2), (55, 128, 4.0, 3), (55, 128, 20.0, 4), (17, 33, 40.0, 5),
          (33, 65, 3.0, 6)]


def _random_cases() -> List[Case]:
    cases = [Case(f"rand-{h}x{w}-s{sigma:g}-{seed}", gaussian(h, w, sigma, seed)[None], True)
             for h, w, sigma, seed in RANDOM]
    by = {c.name: c.flow[0] for c in cases}
    # two images of one batch are independent
    cases.append(Case("batch2-55x128", np.stack([by["rand-55x128-s4-3"], by["rand-55x128-s20-4"]]), True))
    # more images, each a different field (sigma 3 .. 10), with a ragged last workgroup and a partial second tile each
    cases.append(Case("batch8-33x65", np.stack([gaussian(33, 65, 3.0 + k, 6 + k) for k in range(8)]), True))
    return cases


def _edge_cases() -> List[Case]:
    cases = []
    # dyadic flow: every distance is exact in float64 and 13 of the 117 queries have an exact tie
    tie = (np.random.default_rng(9).integers(-12, 13, (2, 9, 13)) / 4).astype(np.float32)
    cases.append(Case("tie-9x13", tie[None], False))
    cases.append(Case("none-landed", np.full((1, 2, 6, 9), 1000.0, np.float32), False))
    one = np.full((2, 6, 9), 1000.0, np.float32)
    one[:, 3, 4] = (0.25, -0.5)
    cases.append(Case("one-landed", one[None], False))
    const = np.empty((1, 2, 7, 10), np.float32)
    const[:, 0], const[:, 1] = 0.5, 0.25
    cases.append(Case("constant", const, False))
    cases.append(Case("zero-flow", np.zeros((1, 2, 7, 10), np.float32), False))
    bad = gaussian(12, 19, 2.0, 21)
    bad[:, 0, 0] = np.nan
    bad[0, 5, 7], bad[1, 5, 8] = np.nan, np.nan
    bad[0, 6, 3], bad[1, 2, 2] = np.inf, np.inf
    bad[0, 9, 11], bad[1, 11, 18] = -np.inf, -np.inf
    bad[:, 4, 4] = (np.inf, np.nan)
    cases.append(Case("nonfinite-12x19", bad[None], True))
    # H = 1 / W = 1: the one row / column stays in frame for flows in (0, 1) across it
    rng = np.random.default_rng(31)
    row = np.stack([rng.standard_normal((1, 37)) * 2.0, rng.uniform(0.1, 0.9, (1, 37))]).astype(np.float32)
    col = np.stack([rng.uniform(0.1, 0.9, (29, 1)), rng.standard_normal((29, 1)) * 2.0]).astype(np.float32)
    cases.append(Case("row-1x37", row[None], True))
    cases.append(Case("col-29x1", col[None], True))
    return cases


CASES: List[Case] = _random_cases() + _edge_cases()
CASE_IDS = [c.name for c in CASES]
BY_NAME: Dict[str, Case] = {c.name: c for c in CASES}
NONFINITE_SOURCES = [(0, 0), (5, 7), (5, 8), (6, 3), (2, 2), (9, 11), (11, 18), (4, 4)]  # (y, x) planted above

_EXPECTED: Dict[str, np.ndarray] = {}


def expected(case: Case) -> np.ndarray:
    """The case's (B, 2, H, W) float32 reference output, computed once per process (treat it as read-only). Building it
    asserts the gap bound of a random case."""
    if case.name not in _EXPECTED:
        outs, gaps = zip(*(interpolate64(img) for img in case.flow))
        if case.random:
            assert min(gaps) >= MIN_GAP, (case.name, min(gaps), "near-tie in a random case: change its seed")
        ref = np.stack(outs)
        ref.setflags(write=False)
        _EXPECTED[case.name] = ref
    return _EXPECTED[case.name]


def landed_count(flow: np.ndarray) -> int:
    """Landed sources of one (2, H, W) image."""
    _, h, w = flow.shape
    with np.errstate(invalid="ignore"):
        x1 = np.arange(w)[None, :] + flow[0].astype(np.float64)
        y1 = np.arange(h)[:, None] + flow[1].astype(np.float64)
        return int(((x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)).sum())


def tie_count(flow: np.ndarray) -> int:
    """Queries of one (2, H, W) image whose least squared distance is attained by more than one landed source."""
    _, h, w = flow.shape
    n = h * w
    s = np.arange(n)
    gx, gy = (s % w).astype(np.float64), (s // w).astype(np.float64)
    x1, y1 = gx + flow[0].reshape(n).astype(np.float64), gy + flow[1].reshape(n).astype(np.float64)
    landed = (x1 > 0) & (x1 < w) & (y1 > 0) & (y1 < h)
    d2 = (gx[:, None] - x1[None, landed]) ** 2 + (gy[:, None] - y1[None, landed]) ** 2
    return int(((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
