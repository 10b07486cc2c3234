"""CPU checks of the on-the-fly correlation forward's references (tests/corr_otf_forward_cases.py): the float64
reference equals the reference project's dense definition where the fp16 path is exact, the calibrated K of the GPU
tolerance is re-measured on the fp32 CPU composition, the host restatement of the kernel's segment rule (the path
census) shows that the cases take every path they claim, the exact form of the prepare step's arithmetic does what its
planted values are there for, and the tolerance catches three kinds of small kernel error. No kernel is launched here."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import corr_backward_cases as cc
import corr_otf_backward_cases as oc
import corr_otf_forward_cases as fc


def _dims(case):
    _, (h, w), levels, _, _, _ = case
    return cc.level_dims(h, w, levels)


# ----------------------------------------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------------------------------------
def test_forward64_equals_the_dense_definition_on_dyadic_inputs():
    """Integer features and C = 64: fmap1 / sqrt(C) and every pooled level are exact in fp16, and half-pixel fractions
    are exact in fp32, so the fp16 path is the dense composition matmul / sqrt(C), avg_pool2d of the volume, window
    lookup, and every sum is exact in float64: the two must be equal, not close."""
    r, (h, w), levels, c = fc.DYADIC
    f1, f2, coords, _ = oc.dyadic_inputs()
    for prepare in (fc.prepare_exact, oc.prepare_emulated):
        f1h, f2h = prepare(f1, f2, levels)
        got = fc.forward64(f1h, f2h, coords, r)
        want = fc.dense_definition64(f1, f2, coords, levels, r)
        assert got.shape == want.shape == (oc.BATCH, levels * (2 * r + 1) ** 2, h, w)
        live = fc.bound64(f1h, f2h, coords, r) > 0  # (a third of the outputs: the coordinates range past the borders)
        assert int(live.sum()) > want.numel() // 4 and int((want != 0).sum()) > int(live.sum()) // 2
        assert torch.equal(got, want), float((got - want).abs().max())


def test_dyadic_inputs_keep_every_partial_sum_exact_in_fp32():
    """The condition the GPU's bit-for-bit test relies on, from the float64 bound: every partial sum is a multiple of
    2^-m and stays below 2^(24-m)."""
    r, _, levels, _ = fc.DYADIC
    f1, f2, coords, _ = oc.dyadic_inputs()
    f1h, f2h = fc.prepare_exact(f1, f2, levels)
    m = fc.DYADIC_QUANTUM_BITS
    ref, bound = fc.forward64(f1h, f2h, coords, r), fc.bound64(f1h, f2h, coords, r)
    assert float(bound.max()) < 2.0 ** (24 - m), float(bound.max())
    assert torch.equal(ref * 2.0**m, torch.round(ref * 2.0**m))
    assert torch.equal(ref.float().double(), ref)
    assert torch.equal(fc.composition32(f1h, f2h, coords, r).double(), ref)  # so the fp32 composition is exact too


@functools.lru_cache(maxsize=None)
def _evaluated(index):
    """(f1h, f2h, coords, reference, bound, fp32 composition) of one case at the prepare step's exact emulation."""
    case = fc.CASES[index]
    r, _, levels, _, _, _ = case
    f1, f2, coords = fc.inputs(case)
    f1h, f2h = fc.prepare_exact(f1, f2, levels)
    return (f1h, f2h, coords, fc.forward64(f1h, f2h, coords, r), fc.bound64(f1h, f2h, coords, r),
            fc.composition32(f1h, f2h, coords, r).double())


def _ratio(got, ref, bound):
    live = bound > 0
    return float(((got - ref).abs()[live] / (fc.EPS24 * bound[live])).max())


def test_calibrated_k_is_the_fp32_compositions_worst_ratio():
    """K_FWD = 4 x the worst |err| / (2^-24 * bound) of the fp32 CPU composition against float64 over all forward cases.
    The recorded ratio must cover a re-measurement (another BLAS may sum in another order: it may be up to 2 x larger
    than what this machine measures, never smaller). Every case has live elements; dead ones are exactly 0."""
    worst, dead = 0.0, 0
    for index, cid in enumerate(fc.CASE_IDS):
        _, _, _, ref, bound, got = _evaluated(index)
        live = bound > 0
        assert int(live.sum()) > 0, cid
        assert bool((got[~live] == 0).all()) and bool((ref[~live] == 0).all()), cid
        ratio = _ratio(got, ref, bound)
        print(f"calibration {cid}: {int(live.sum())} live / {int((~live).sum())} dead, worst ratio {ratio:.3f}")
        worst, dead = max(worst, ratio), dead + int((~live).sum())
    print(f"calibration: worst ratio {worst:.3f}, recorded {fc.CALIBRATED_RATIO_FWD} -> K_FWD = {fc.K_FWD:.2f}")
    assert dead > 0 and fc.K_FWD == 4.0 * fc.CALIBRATED_RATIO_FWD
    assert worst <= fc.CALIBRATED_RATIO_FWD <= 2.0 * worst, (worst, fc.CALIBRATED_RATIO_FWD)


def test_case_list_holds_what_the_forward_needs():
    assert [c[:5] for c in fc.CASES[: len(oc.GAUSS_CASES)]] == list(oc.GAUSS_CASES) and len(set(fc.CASE_IDS)) == len(fc.CASES)
    assert fc.CASE_IDS[: len(oc.CASE_IDS)] == oc.CASE_IDS
    own = fc.CASES[len(oc.GAUSS_CASES):]
    assert {k for r, hw, l, c, k, b in own if c == 256 and r == 4 and hw == (17, 37) and l == 4} == {"smooth", "mixed"}
    assert any(b == 3 for *_, b in own)
    assert any(_dims(case)[-1] == (2, 2) for case in own)
    assert {16, 17} <= {hw[1] for _, hw, *_ in own} and {2, 3} <= {hw[0] for _, hw, *_ in own}
    assert {r for r, *_ in fc.CASES} == set(range(5)) and {c for _, _, _, c, _, _ in fc.CASES} == {32, 64, 96, 256}
    for index, case in enumerate(fc.CASES[: len(oc.GAUSS_CASES)]):  # the shared cases run on the backward's own inputs
        assert all(torch.equal(a, b) for a, b in zip(fc.inputs(case), oc.case_inputs(case[:5])[:3])), index


# ----------------------------------------------------------------------------------------------------------
# path census
# ----------------------------------------------------------------------------------------------------------
def _census_by_the_kernels_loop(coords, radius, dims):
    """The segment rule of corr_otf_kernel written as its loops (one segment, one query at a time), in numpy float32."""
    co = coords.numpy().astype(np.float32)
    b, _, h, w = co.shape
    pk = 2 * radius + 2
    segy, segx = -(-h // 2), -(-w // 16)
    out = []
    for l, (hl, wl) in enumerate(dims):
        kind = np.zeros((b, segy, segx), dtype=np.int64)
        area = np.zeros((b, segy, segx), dtype=np.int64)
        inv = np.float32(1.0) / np.float32(1 << l)
        for bi in range(b):
            for sy in range(segy):
                for sx in range(segx):
                    by0 = bx0 = 1 << 29
                    by1 = bx1 = -(1 << 29)
                    for qi in range(32):
                        qy, qx = 2 * sy + qi // 16, 16 * sx + qi % 16
                        if qy >= h or qx >= w:
                            continue
                        cx, cy = co[bi, 0, qy, qx] * inv, co[bi, 1, qy, qx] * inv
                        if not (abs(cx) < np.float32(4194304.0) and abs(cy) < np.float32(4194304.0)):
                            continue
                        xs, ys = int(math.floor(cx)) - radius, int(math.floor(cy)) - radius
                        if ys + pk > 0 and ys < hl and xs + pk > 0 and xs < wl:
                            by0, bx0, by1, bx1 = min(by0, ys), min(bx0, xs), max(by1, ys + pk - 1), max(bx1, xs + pk - 1)
                    by0, bx0, by1, bx1 = max(by0, 0), max(bx0, 0), min(by1, hl - 1), min(bx1, wl - 1)
                    if by1 >= by0 and bx1 >= bx0:
                        area[bi, sy, sx] = (by1 - by0 + 1) * (bx1 - bx0 + 1)
                        kind[bi, sy, sx] = fc.BOX if area[bi, sy, sx] <= 384 else fc.PER_QUERY
        out.append((kind, area))
    return out


@pytest.mark.parametrize("cid", ["r4-5x13-L2-C32-mixed", "r2-6x17-L2-C32-mixed", "r4-17x37-L4-C64-away"])
def test_census_is_the_kernels_segment_rule(cid):
    case = fc.CASES[fc.CASE_IDS.index(cid)]
    coords = fc.inputs(case)[2]
    if cid.endswith("away"):
        coords, _ = cc.with_specials(coords, case[2])  # NaN, inf and the 2^22 edges go through the same rule
    for got, (kind, area) in zip(fc.census(coords, case[0], _dims(case)), _census_by_the_kernels_loop(coords, case[0], _dims(case))):
        assert np.array_equal(got["kind"], kind) and np.array_equal(got["area"], area)
        assert np.array_equal(got["rows"] * got["cols"], area)


def test_cases_take_every_path_they_claim():
    """All three (segment, level) kinds occur many times over the case set, and each case that is there for a path
    takes it."""
    total = np.zeros(3, dtype=np.int64)
    counts = {}
    for case, cid in zip(fc.CASES, fc.CASE_IDS):
        counts[cid] = fc.census_counts(fc.census(fc.inputs(case)[2], case[0], _dims(case)))
        total += np.array(counts[cid]).sum(axis=0)
        print(f"census {cid}: per level (all-outside, box, per-query) = {counts[cid]}")
    print(f"census: {total[0]} all-outside, {total[1]} box-pass, {total[2]} per-query (segment, level) pairs")
    assert total[fc.OUTSIDE] >= 100 and total[fc.BOX] >= 1000 and total[fc.PER_QUERY] >= 200, total
    for cid, per_level in counts.items():
        if "17x37" in cid and cid.endswith("mixed"):  # scattered windows: per-query at level 0, box passes above it
            assert per_level[0][fc.PER_QUERY] >= 50 and all(c[fc.BOX] == 54 for c in per_level[1:]), (cid, per_level)
        if cid.endswith("still"):
            assert all(c == (0, 54, 0) for c in per_level), (cid, per_level)
        if cid.endswith("away"):  # two segments in three are outside every level
            assert all(c[fc.OUTSIDE] == 36 for c in per_level), (cid, per_level)
        if "smooth" in cid and cid.startswith("r4-17x37"):  # radius 4's wider windows: both paths at level 0
            assert per_level[0][fc.BOX] > 0 and per_level[0][fc.PER_QUERY] > 0, (cid, per_level)
    assert counts["r0-17x37-L4-C64-smooth"][3][fc.OUTSIDE] == 4


def test_census_of_the_path_grid_pairs():
    """The all-fit / none-fit pair of the neighbour-independence test and the 384 / 396 pair of the kTMax-edge test."""
    g = fc.PATH_GRID
    dims = cc.level_dims(g["h"], g["w"], g["levels"])
    assert dims[0][0] * dims[0][1] > fc.T_MAX and dims[1][0] * dims[1][1] > fc.T_MAX >= dims[2][0] * dims[2][1]
    segs = (g["h"] // 2) * (g["w"] // 16)
    run_a = fc.census_counts(fc.census(fc.still_coords(), g["radius"], dims))
    coords_b, moved = fc.scattered_coords()
    run_b = fc.census_counts(fc.census(coords_b, g["radius"], dims))
    print(f"census run A (still): {run_a}; run B (two queries per segment in opposite corners): {run_b}")
    assert run_a == [(0, segs, 0)] * 3
    assert run_b == [(0, 0, segs), (0, 0, segs), (0, segs, 0)]
    assert int(moved.sum()) == 2 * segs
    inside = (coords_b[0, 0] >= 0) & (coords_b[0, 0] <= g["w"] - 1) & (coords_b[0, 1] >= 0) & (coords_b[0, 1] <= g["h"] - 1)
    assert bool(inside[moved].all())  # moved, but still inside the level
    assert torch.equal(coords_b[:, :, ~moved], fc.still_coords()[:, :, ~moved])

    sy, sx = fc.KTMAX_SEGMENT
    fit, touched7 = fc.ktmax_coords(7)
    over, touched8 = fc.ktmax_coords(8)
    cen7, cen8 = fc.census(fit, g["radius"], dims), fc.census(over, g["radius"], dims)
    a7 = {k: int(v[0, sy, sx]) for k, v in cen7[0].items()}
    a8 = {k: int(v[0, sy, sx]) for k, v in cen8[0].items()}
    print(f"census kTMax edge: +7 columns {a7}, +8 columns {a8}")
    assert a7 == {"kind": fc.BOX, "area": 384, "rows": 12, "cols": 32}
    assert -(-a7["area"] // 16) == 24 and a7["area"] - 1 == 383  # nT = 24: every wave's six N-tiles; last column 383
    assert a8 == {"kind": fc.PER_QUERY, "area": 396, "rows": 12, "cols": 33}
    assert fc.census_counts(cen7) == [(0, segs, 0)] * 3  # every other (segment, level) of both inputs is a box pass
    assert fc.census_counts(cen8) == [(0, segs - 1, 1), (0, segs, 0), (0, segs, 0)]
    assert torch.equal(touched7, touched8) and int(touched7.sum()) == 2
    assert torch.equal(fit[:, :, ~touched7], over[:, :, ~touched7])
    assert torch.equal(fit, torch.round(fit)) and torch.equal(over, torch.round(over))


# ----------------------------------------------------------------------------------------------------------
# the prepare step's arithmetic
# ----------------------------------------------------------------------------------------------------------
def test_prepare_scale_is_the_fp32_form():
    """1.0f / sqrtf((float)C) differs from fp32(1 / sqrt(C)) computed in double by one ulp at C = 96, 288, 384, 448
    (C % 32 == 0, C <= 512): why ``prepare_exact`` exists beside ``oc.prepare_emulated``."""
    differ = [c for c in range(32, 513, 32) if float(fc.prepare_scale(c)) != float(np.float32(1.0 / math.sqrt(c)))]
    assert differ == [96, 288, 384, 448], differ
    for c in differ:
        a, b = fc.prepare_scale(c), np.float32(1.0 / math.sqrt(c))
        assert np.nextafter(a, b) == b
    assert float(fc.prepare_scale(64)) == 0.125 and float(fc.prepare_scale(256)) == 0.0625
    assert {c for c, *_ in fc.PREPARE_CASES} == {32, 96, 160, 256}
    assert {hw for _, hw, _, _ in fc.PREPARE_CASES} == {(17, 37), (5, 13), (9, 35), (2, 2)}
    assert {b for _, _, b, _ in fc.PREPARE_CASES} == {1, 3} and {l for *_, l in fc.PREPARE_CASES} == {1, 2, 3, 4}
    assert all((h * w) % 64 != 0 for _, (h, w), _, _ in fc.PREPARE_CASES)


def test_planted_values_reach_the_fp16_edges_they_are_there_for():
    c, (h, w), b, levels = fc.PLANTED
    f1, f2 = fc.planted_inputs()
    vals = torch.tensor(fc.planted_values())
    n = vals.numel()
    f1h, f2h = fc.prepare_exact(f1, f2, levels)
    for got in (f1h[0, :, :, 5].reshape(-1)[:n], f2h[0][0, :, :, 3].reshape(-1)[:n]):
        assert torch.equal(got.view(torch.int16), vals.half().view(torch.int16))  # (1 / sqrt(64) is exact)
    got = f2h[0][0, :, :, 3].reshape(-1)[:n].double()
    assert math.copysign(1.0, float(got[0])) == -1.0 and float(got[0]) == 0.0  # -0.0 keeps its sign
    sub = (got.abs() > 0) & (got.abs() < 2.0**-14)
    assert int(sub.sum()) >= 6 and int(((vals != 0) & (got == 0)).sum()) >= 2  # subnormals; ties / underflow to zero
    assert int(torch.isinf(got).sum()) == 2 and int((got.abs() == 65504.0).sum()) == 3
    t = 2.0**-11
    assert [float(v) for v in torch.tensor([1 + t, 1 + 3 * t, 2049.0, 2051.0]).half()] == [1.0, 1 + 4 * t, 2048.0, 2052.0]
    for ch, want in ((7, 1.0), (8, 1 + 4 * t), (9, -2.0)):  # ties formed by the pooling, rounded to even once
        assert float(f2h[1][1, 0, 0, ch]) == want and float(f2h[2][2, 0, 0, ch]) == want
        early = torch.nn.functional.avg_pool2d(f2[:, ch : ch + 1].half().float(), 2, stride=2).half()
        assert float(early[1, 0, 0, 0]) != want  # rounding before the pool gives another value


# ----------------------------------------------------------------------------------------------------------
# sensitivity of the tolerance
# ----------------------------------------------------------------------------------------------------------
def _shiftable_level(case):
    """The highest level whose target count is no multiple of 16 (its last N-tile is partial), or None."""
    ragged = [l for l, (hl, wl) in enumerate(_dims(case)) if (hl * wl) % 16 != 0]
    return ragged[-1] if ragged else None


@pytest.mark.parametrize("what", ["weight", "drop_corner", "shift_target"])
def test_tolerance_catches_small_kernel_errors(what):
    """The fp32 CPU composition broken the way a kernel bug would break it -- one bilinear weight scaled by 1 + 1e-3; the
    (y + 1, x + 1) tap dropped where it lands on the last level's corner; the last target of a partial N-tile reading
    its neighbour -- exceeds K_FWD * 2^-24 * bound on every case it applies to, by orders of magnitude, and among the
    elements it flags are ones off by less than the 2e-2 the dense-oracle comparison (tests/test_gpu_otf.py) allows."""
    worst, applied = [], 0
    for index, (case, cid) in enumerate(zip(fc.CASES, fc.CASE_IDS)):
        r, _, levels, _, _, _ = case
        f1h, f2h, coords, ref, bound, clean = _evaluated(index)
        perturb = {"weight": {"weight": 1.0 + 1e-3}, "drop_corner": {"drop_corner": levels - 1},
                   "shift_target": {"shift_target": _shiftable_level(case)}}[what]
        if perturb.get("shift_target", 0) is None:
            continue
        got = fc.composition32(f1h, f2h, coords, r, perturb).double()
        if torch.equal(got, clean):
            continue  # (no window of this case reaches the broken tap)
        applied += 1
        err = (got - ref).abs()
        flagged = err > fc.tolerance(bound)
        ratio = _ratio(got, ref, bound)
        small = int((flagged & (err <= 2e-2)).sum())
        print(f"sensitivity {what} {cid}: ratio {ratio:.3g} (K_FWD = {fc.K_FWD:.2f}), {int(flagged.sum())} elements over "
              f"tolerance, {small} of them within 2e-2; max |d| {float(err.max()):.2e}, mean |d| {float(err.mean()):.2e}")
        assert ratio > fc.K_FWD and small > 0, (cid, ratio)
        worst.append(ratio)
    print(f"sensitivity {what}: {applied} cases, ratio {min(worst):.3g} .. {max(worst):.3g}")
    assert applied >= len(fc.CASES) // 2
