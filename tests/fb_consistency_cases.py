"""Float64 reference and the case table of the fb_consistency tests (csrc/fb_consistency.hip,
optical_flow.fb_consistency). NumPy only; every input comes from a seeded generator or is written out. Not a test module.

The reference states the contract of include/oflow.h (oflow_fb_consistency_f32) in float64, evaluated AT THE FP32-ROUNDED
px, py: the sampling position is formed in fp32 exactly as an implementation forms it (one fp32 sum per axis), so the
inside test, floor, the tap indices and the weights (px - floor(px) is exact) agree with an implementation bit for bit
and only the interpolation and residual arithmetic differ. The bilinear value is formed as the contract writes it,
top + wy * (bot - top) with top = t00 + wx * (t01 - t00): a non-finite tap gives NaN even under a zero weight, so
every non-finite tap makes its pixel occluded.

Tolerance of `err` for an fp32 implementation, derived (DESIGN.md §4 "fb_consistency"), not tuned: with T the largest
|tap| the pixel reads and eps = 2^-24, one lerp of values within [-T, T] rounds three times on magnitudes <= 2T, 2T, T:
<= 5 eps T; the second level carries that and adds its own: s is within 10 eps T; u + s within 11 eps (|u| + T); its
square within 23 eps (|u| + T)^2; the sum of both squares and its rounding within 24 eps ((|u|+T)^2 + (|v|+T)^2)
<= 48 eps (|u| + |v| + T)^2 < E = 2^-18 (|u| + |v| + T)^2. FMA contraction only removes roundings.

Masks are compared exactly except on EXEMPT pixels, |err64 - thr64| <= 2 E, where an error of E in err (and the far
smaller one in thr) can legitimately move the pixel across the threshold. Building a case's reference asserts, on the
CPU, that at most MAX_EXEMPT = 0.5 % of its pixels are exempt and, for a random case, that at least MIN_CLASS = 10 % of
its inside pixels fall in each class, so the masks are a real test in both directions.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple

import numpy as np

MAX_EXEMPT = 0.005
MIN_CLASS = 0.10
ALPHA, BETA = 0.01, 0.5  # UnFlow's defaults (the operator's too)


class Case(NamedTuple):
    name: str
    fw: np.ndarray  # (B, 2, H, W) float32
    bw: np.ndarray  # (B, 2, H, W) float32
    alpha: float
    beta: float
    random: bool  # the class-balance assertion applies (both directions)


class Ref(NamedTuple):
    mask: np.ndarray  # (B, 1, H, W) bool
    err: np.ndarray  # (B, 1, H, W) float64: +inf outside, NaN where a tap is not finite
    thr: np.ndarray  # (B, 1, H, W) float64 (NaN outside)
    tol: np.ndarray  # (B, 1, H, W) float64: E (0 outside)
    inside: np.ndarray  # (B, 1, H, W) bool
    exempt: np.ndarray  # (B, 1, H, W) bool: the mask is not compared here


def check64(a: np.ndarray, o: np.ndarray, alpha: float, beta: float) -> Ref:
    """One direction of the contract: flow ``a`` checked against the other flow ``o``, both (B, 2, H, W) fp32."""
    assert a.dtype == o.dtype == np.float32 and a.shape == o.shape and a.ndim == 4 and a.shape[1] == 2
    b, _, h, w = a.shape
    u, v = a[:, 0], a[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        px = np.arange(w, dtype=np.float32)[None, None, :] + u  # fp32 sums, rounded once
        py = np.arange(h, dtype=np.float32)[None, :, None] + v
        assert px.dtype == py.dtype == np.float32
        inside = (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)  # false for NaN
    pxs, pys = np.where(inside, px, 0).astype(np.float64), np.where(inside, py, 0).astype(np.float64)
    fx, fy = np.floor(pxs), np.floor(pys)
    wx, wy = pxs - fx, pys - fy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    bi = np.arange(b)[:, None, None]
    u64, v64 = u.astype(np.float64), v.astype(np.float64)
    tmax = np.zeros((b, h, w))
    s = []
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(2):
            plane = o[:, c].astype(np.float64)
            t00, t01, t10, t11 = plane[bi, y0, x0], plane[bi, y0, x1], plane[bi, y1, x0], plane[bi, y1, x1]
            top = t00 + wx * (t01 - t00)
            bot = t10 + wx * (t11 - t10)
            s.append(top + wy * (bot - top))
            for t in (t00, t01, t10, t11):
                tmax = np.maximum(tmax, np.abs(t))  # (NaN propagates: such a pixel has no tolerance, and needs none)
        err = (u64 + s[0]) ** 2 + (v64 + s[1]) ** 2
        thr = alpha * (u64 * u64 + v64 * v64 + s[0] ** 2 + s[1] ** 2) + beta
        mask = ~(err <= thr) | ~inside
        tol = 2.0 ** -18 * (np.abs(u64) + np.abs(v64) + tmax) ** 2
        exempt = inside & (np.abs(err - thr) <= 2 * tol)  # (false for NaN)
    err = np.where(inside, err, np.inf)
    thr = np.where(inside, thr, np.nan)
    tol = np.where(inside & np.isfinite(tol), tol, 0.0)
    return Ref(*(x[:, None] for x in (mask, err, thr, tol, inside, exempt)))


# ---------------------------------------------------------------------------------------------------- construction
def smooth(h: int, w: int, amp: float, seed: int) -> np.ndarray:
    """A smooth (2, h, w) float64 field of amplitude ~amp: a seeded normal grid of 4-px cells, bilinearly upsampled."""
    gh, gw = h // 4 + 2, w // 4 + 2
    g = np.random.default_rng(seed).standard_normal((2, gh, gw)) * amp
    y, x = np.arange(h) / 4.0, np.arange(w) / 4.0
    yi, xi = y.astype(int), x.astype(int)
    fy, fx = (y - yi)[None, :, None], (x - xi)[None, None, :]
    g00, g01 = g[:, yi][:, :, xi], g[:, yi][:, :, xi + 1]
    g10, g11 = g[:, yi + 1][:, :, xi], g[:, yi + 1][:, :, xi + 1]
    return (g00 * (1 - fx) + g01 * fx) * (1 - fy) + (g10 * (1 - fx) + g11 * fx) * fy


def pair(h: int, w: int, t, amp: float, seed: int):
    """(fw, bw) (2, h, w) fp32: the translation ``t`` = (tx, ty) and its exact inverse -- a constant translation is
    exactly consistent -- plus smooth noise of amplitude ``amp`` on both, which moves pixels across the threshold (the
    amplitudes in the table below were chosen for the class balance ``expected`` asserts, from this reference alone)."""
    tv = np.asarray(t, np.float64).reshape(2, 1, 1)
    fw = np.ascontiguousarray((tv + smooth(h, w, amp, seed)).astype(np.float32))
    bw = np.ascontiguousarray((-tv + smooth(h, w, amp, seed + 1000)).astype(np.float32))
    return fw, bw


def _batch(pairs):
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _random_cases() -> List[Case]:
    cases = []
    # 13x17, batch 3: odd W, H*W = 221 = 1 mod 4: images 1 and 2 start off the 16-byte alignment, a 1-pixel tail run
    cases.append(Case("rand-13x17-b3", *_batch([pair(13, 17, (1.5, -0.75), 1.0, 1), pair(13, 17, (-2.0, 1.25), 1.0, 2),
                                                pair(13, 17, (0.25, 0.5), 1.0, 3)]), ALPHA, BETA, True))
    # 33x65: W = 1 mod 4 and mod 64, 2145 pixels = three workgroups, the last one ragged
    cases.append(Case("rand-33x65", *_batch([pair(33, 65, (3.25, -1.5), 1.0, 4)]), ALPHA, BETA, True))
    # 16x64: every run whole and aligned (fully vectorised rows), batch 2 for the image stride
    cases.append(Case("rand-16x64-b2", *_batch([pair(16, 64, (-2.5, 0.75), 1.0, 5), pair(16, 64, (6.0, 2.0), 1.2, 6)]),
                      ALPHA, BETA, True))
    # the threshold's two parameters: a loose one on the 13x17 fields ...
    by = cases[0]
    cases.append(Case("rand-13x17-b3-a0.05-b1", by.fw, by.bw, 0.05, 1.0, True))
    # ... and (0, 0): thr = 0, occluded = err > 0, which holds for every inside pixel of these fields by a wide margin
    # (a pixel with err = thr = 0 exactly would be exempt by the rule above, so no consistent class can be tested here)
    cases.append(Case("rand-13x17-b3-a0-b0", by.fw, by.bw, 0.0, 0.0, False))
    return cases


# the written-out half-pixel case: fw = (0.5, 0) everywhere, bw = (-0.5 - 0.25 j, 0) at column j, 4 x 8. Pixel (i, j) with
# j <= 6 samples s0 = (bw[j] + bw[j+1]) / 2 = -0.5 - 0.25 (j + 0.5): err = (0.25 j + 0.125)^2, all dyadic, exact in fp32
# and fp64; thr = 0.01 (0.25 + s0^2) + 0.5 lies in (0.5, 0.55), so columns 0..2 are consistent (err <= 0.390625),
# columns 3..6 occluded (err >= 0.765625); column 7 lands at 7.5 > W - 1: outside.
HALF_PIXEL_ERR = [(0.25 * j + 0.125) ** 2 for j in range(7)] + [np.inf]
HALF_PIXEL_MASK = [False, False, False, True, True, True, True, True]

# the frame-edge case (5 x 9, bw = 0 so err = u^2 + v^2 where inside): (i, j, u, v, inside). Every px, py below is exact
# in fp32, so "on the edge" and "one ulp beyond it" are what the kernel sees.
_UP = np.nextafter(np.float32(8.0), np.float32(np.inf))  # the next fp32 after W - 1 = 8
_UP_Y = np.nextafter(np.float32(4.0), np.float32(np.inf))  # the next fp32 after H - 1 = 4
_DOWN = np.nextafter(np.float32(-1.0), np.float32(-np.inf))  # 1 + _DOWN = -2^-23: the fp32 sum is exact
EDGE_PIXELS = [
    (0, 3, -3.0, 0.0, True),  # lands exactly on x = 0
    (0, 5, 3.0, 0.0, True),  # exactly on x = W - 1
    (2, 4, 0.0, -2.0, True),  # exactly on y = 0
    (2, 6, 0.0, 2.0, True),  # exactly on y = H - 1
    (4, 8, -8.0, -4.0, True),  # the far corner onto the origin
    (0, 0, 8.0, 4.0, True),  # the origin onto the far corner
    (1, 1, float(_DOWN), 0.0, False),  # x = -2^-23: one ulp (of 1) below 0
    (1, 0, float(_UP), 0.0, False),  # x = nextafter(W - 1)
    (1, 4, 0.0, float(_DOWN), False),  # y = -2^-23
    (0, 7, 0.0, float(_UP_Y), False),  # y = nextafter(H - 1)
    (3, 3, -3.5, 0.0, False),  # half a pixel out
    (3, 5, 0.0, 1.75, False),
]

# non-finite entries planted in the 13x17 field of seed 1: (channel, i, j, value), in fw (own flow: the pixel is outside)
# and in bw (a tap: every pixel whose four taps include it gets a NaN residual)
NONFINITE_FW = [(0, 2, 3, np.nan), (1, 5, 5, np.nan), (0, 7, 9, np.inf), (1, 9, 2, -np.inf), (0, 11, 15, -np.inf)]
NONFINITE_BW = [(0, 4, 8, np.nan), (1, 6, 12, np.inf), (0, 10, 4, -np.inf)]


def _edge_cases() -> List[Case]:
    cases = []
    z = np.zeros((1, 2, 7, 10), np.float32)
    cases.append(Case("zero-flow-7x10", z, z.copy(), ALPHA, BETA, False))
    fw = np.zeros((1, 2, 4, 8), np.float32)
    fw[:, 0] = 0.5
    bw = np.zeros((1, 2, 4, 8), np.float32)
    bw[:, 0] = -0.5 - 0.25 * np.arange(8, dtype=np.float32)
    cases.append(Case("half-pixel-4x8", fw, bw, ALPHA, BETA, False))
    fw = np.zeros((1, 2, 5, 9), np.float32)
    for i, j, u, v, _ in EDGE_PIXELS:
        fw[0, :, i, j] = (u, v)
    cases.append(Case("frame-edge-5x9", fw, np.zeros_like(fw), ALPHA, BETA, False))
    fw, bw = (x.copy()[None] for x in pair(13, 17, (1.5, -0.75), 1.0, 1))
    for c, i, j, val in NONFINITE_FW:
        fw[0, c, i, j] = val
    for c, i, j, val in NONFINITE_BW:
        bw[0, c, i, j] = val
    cases.append(Case("nonfinite-13x17", fw, bw, ALPHA, BETA, False))
    # degenerate shapes. 1x1: only a zero flow stays inside (image 0), anything else leaves (image 1)
    one = np.zeros((2, 2, 1, 1), np.float32)
    one[1, :, 0, 0] = (0.25, 0.0)
    cases.append(Case("one-pixel-1x1-b2", one, np.zeros_like(one), ALPHA, BETA, False))
    # one row (v = 0: py = 0 = H - 1, y0 = y1 = 0) and one column (u = 0)
    fw, bw = pair(1, 7, (1.0, 0.0), 0.5, 11)
    fw[1], bw[1] = 0.0, 0.0
    cases.append(Case("row-1x7", fw[None], bw[None], ALPHA, BETA, False))
    fw, bw = pair(5, 1, (0.0, -1.0), 0.5, 12)
    fw[0], bw[0] = 0.0, 0.0
    cases.append(Case("col-5x1", fw[None], bw[None], ALPHA, BETA, False))
    return cases


CASES: List[Case] = _random_cases() + _edge_cases()
for _c in CASES:  # the C ABI tests hand the arrays' memory to the kernel as it is
    assert _c.fw.flags["C_CONTIGUOUS"] and _c.bw.flags["C_CONTIGUOUS"] and _c.fw.dtype == _c.bw.dtype == np.float32, _c.name
CASE_IDS = [c.name for c in CASES]
BY_NAME: Dict[str, Case] = {c.name: c for c in CASES}

_EXPECTED: Dict[str, tuple] = {}


def expected(case: Case):
    """(Ref of fw checked against bw, Ref of bw checked against fw), computed once per process (read-only). Building them
    asserts the exemption cap and, for a random case, the class balance."""
    if case.name not in _EXPECTED:
        refs = (check64(case.fw, case.bw, case.alpha, case.beta), check64(case.bw, case.fw, case.alpha, case.beta))
        for d, r in zip(("fw", "bw"), refs):
            n = r.mask.size
            assert r.exempt.sum() <= MAX_EXEMPT * n, (case.name, d, int(r.exempt.sum()), n, "too many exempt pixels")
            if case.random:
                ins = int(r.inside.sum())
                occ = int((r.mask & r.inside).sum())
                assert ins >= 0.3 * n, (case.name, d, ins, n, "too few inside pixels")
                assert MIN_CLASS * ins <= occ <= (1 - MIN_CLASS) * ins, (case.name, d, occ, ins, "unbalanced classes")
            for x in r:
                x.setflags(write=False)
        _EXPECTED[case.name] = refs
    return _EXPECTED[case.name]


def compare(case: Case, direction: int, mask: np.ndarray, err=None) -> None:
    """Assert an implementation's (B, 1, H, W) bool mask, and fp32 residual if given, of one direction (0: fw) against the
    reference: the mask exactly outside the exempt pixels, the residual within E where it is finite, the same
    non-finite kind (+inf outside the frame, NaN from a non-finite tap) elsewhere."""
    r = expected(case)[direction]
    tag = (case.name, "fw" if direction == 0 else "bw")
    assert mask.shape == r.mask.shape and mask.dtype == np.bool_, tag
    bad = (mask != r.mask) & ~r.exempt
    assert not bad.any(), (*tag, "mask differs at", np.argwhere(bad)[:5].tolist())
    if err is None:
        return
    assert err.shape == r.err.shape and err.dtype == np.float32, tag
    fin = np.isfinite(r.err)
    assert np.array_equal(np.isnan(err), np.isnan(r.err)), (*tag, "NaN pattern")
    assert np.array_equal(np.isposinf(err), np.isposinf(r.err)), (*tag, "+inf pattern")
    diff = np.abs(err[fin].astype(np.float64) - r.err[fin])
    over = diff > r.tol[fin]
    assert not over.any(), (*tag, "err off by", float(diff[over].max()), "allowed", float(r.tol[fin][over].min()))
