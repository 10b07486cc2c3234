"""The on-the-fly (fp16, volume-free) correlation forward (csrc/corr_otf.hip) against float64: the MFMA window lookup
through ``torch.ops.oflow.corr_lookup_otf`` and through the C ABI on every path the kernel has (box pass, per-query
passes, the zero fill; the census of tests/corr_otf_forward_cases.py says which input takes which), and the prepare
step bit for bit. References and inputs: tests/corr_otf_forward_cases.py (checked on the CPU by
tests/test_corr_otf_forward_host.py).

Tolerance: the fp16 tensors the prepare op returned are the operands, so only the kernel's own fp32 arithmetic is left:
per element |got - ref| <= K_FWD * 2^-24 * bound + 1e-30 with bound = the reference pipeline on |f1h|, |f2h[l]| and
K_FWD = 4 x the worst ratio of the same composition run in fp32 on the CPU (K_FWD = 18.88; calibrated on that
composition, never on the kernel); exactly 0 where the bound is 0. On dyadic inputs the output equals float64 bit for
bit, and a query's output has the same bits whichever pass computed it.
"""
from __future__ import annotations

import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import corr_backward_cases as cc
import corr_otf_backward_cases as oc
import corr_otf_forward_cases as fc
from optical_flow import _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OPS = torch.ops.oflow
NAN = float("nan")
E_NULL, E_SHAPE, E_LEVELS, E_TINY, E_RADIUS = -1, -2, -3, -4, -5
GUARD = 4096  # elements in front of and behind every carved buffer


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    _native.load()


def _prepared(f1, f2, levels):
    f1h, f2h = OPS.corr_otf_prepare(f1.to(DEV), f2.to(DEV), levels)
    return f1h, list(f2h)


def _host(f1h, f2h):
    return f1h.cpu(), [t.cpu() for t in f2h]


@functools.lru_cache(maxsize=None)
def _case(index):
    """The fp16 tensors the prepare op returned (on the device), the coordinates, and the float64 reference / bound
    from those tensors copied to the host."""
    case = fc.CASES[index]
    r, _, levels, _, _, _ = case
    f1, f2, coords = fc.inputs(case)
    f1h, f2h = _prepared(f1, f2, levels)
    host = _host(f1h, f2h)
    return r, f1h, f2h, coords, fc.forward64(*host, coords, r), fc.bound64(*host, coords, r)


@functools.lru_cache(maxsize=None)
def _path_grid():
    g = fc.PATH_GRID
    f1h, f2h = _prepared(*fc.path_grid_features(), g["levels"])
    return g["radius"], f1h, f2h, _host(f1h, f2h)


def _assert_close(got, ref, bound, what):
    assert got.shape == ref.shape and got.dtype == torch.float32, (what, got.shape)
    got = got.cpu().double()
    assert bool(torch.isfinite(got).all()), what
    live = bound > 0
    err = (got - ref).abs()
    worst = float((err[live] / (fc.EPS24 * bound[live])).max())
    print(f"{what}: {int(live.sum())} live / {int((~live).sum())} dead elements, worst |err| / (2^-24 bound) = {worst:.3f}"
          f" (K_FWD = {fc.K_FWD:.2f})")
    assert int(live.sum()) > 0, what
    assert bool((got[~live] == 0).all()), (what, "an element no tap reaches is not exactly 0")
    assert bool((err <= fc.tolerance(bound)).all()), (what, worst)


def _rows(out):
    """(B, L*K*K, H, W) -> (B*H*W, L*K*K): one row per query."""
    return out.permute(0, 2, 3, 1).reshape(-1, out.shape[1])


# ----------------------------------------------------------------------------------------------------------
# parity with float64
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(fc.CASES)), ids=fc.CASE_IDS)
def test_forward_matches_fp64(index):
    r, f1h, f2h, coords, ref, bound = _case(index)
    got = OPS.corr_lookup_otf(f1h, f2h, coords.to(DEV), r)
    _assert_close(got, ref, bound, fc.CASE_IDS[index])


def test_forward_exact_on_dyadic_inputs():
    """Half-pixel coordinates, integer features, C = 64: every product and partial sum is a multiple of 2^-17 below 2^7
    (asserted from the float64 bound), so the output equals float64 bit for bit in any summation order: the index
    mapping with no tolerance to hide in. More than half of the outputs a tap reaches are nonzero (a third of all
    outputs are live: the coordinates range past the borders and the upper levels are smaller than the window)."""
    r, _, levels, _ = fc.DYADIC
    f1, f2, coords, _ = oc.dyadic_inputs()
    f1h, f2h = _prepared(f1, f2, levels)
    e1h, e2h = fc.prepare_exact(f1, f2, levels)
    assert torch.equal(f1h.cpu(), e1h) and all(torch.equal(a.cpu(), b) for a, b in zip(f2h, e2h))
    ref, bound = fc.forward64(e1h, e2h, coords, r), fc.bound64(e1h, e2h, coords, r)
    m = fc.DYADIC_QUANTUM_BITS
    assert float(bound.max()) < 2.0 ** (24 - m) and torch.equal(ref * 2.0**m, torch.round(ref * 2.0**m))
    live = int((bound > 0).sum())
    assert live > ref.numel() // 4 and int((ref != 0).sum()) > live // 2
    got = OPS.corr_lookup_otf(f1h, f2h, coords.to(DEV), r).cpu().double()
    assert torch.equal(got, ref), (int((got != ref).sum()), float((got - ref).abs().max()))


def test_two_calls_give_the_same_bits():
    r, f1h, f2h, coords, _, _ = _case(fc.CASE_IDS.index("r4-17x37-L4-C64-mixed"))
    co = coords.to(DEV)
    assert torch.equal(OPS.corr_lookup_otf(f1h, f2h, co, r), OPS.corr_lookup_otf(f1h, f2h, co, r))


# ----------------------------------------------------------------------------------------------------------
# the two passes
# ----------------------------------------------------------------------------------------------------------
def test_a_querys_output_does_not_depend_on_its_neighbours():
    """Each C[q, t] is its own k-ordered MFMA chain, so the box pass and the per-query pass must give the same bits.
    Run A: every segment takes the box pass at every level. Run B: two queries of every segment sit in opposite
    corners of the level, so no segment fits at levels 0 and 1 (the census, asserted here and on the CPU). The
    unmoved queries' outputs are bit-identical, and run B as a whole meets the float64 tolerance."""
    r, f1h, f2h, host = _path_grid()
    g = fc.PATH_GRID
    dims = cc.level_dims(g["h"], g["w"], g["levels"])
    segs = (g["h"] // fc.SEG_ROWS) * (g["w"] // fc.SEG_COLS)
    coords_a = fc.still_coords()
    coords_b, moved = fc.scattered_coords()
    assert fc.census_counts(fc.census(coords_a, r, dims)) == [(0, segs, 0)] * 3
    assert fc.census_counts(fc.census(coords_b, r, dims)) == [(0, 0, segs), (0, 0, segs), (0, segs, 0)]
    out_a = OPS.corr_lookup_otf(f1h, f2h, coords_a.to(DEV), r).cpu()
    out_b = OPS.corr_lookup_otf(f1h, f2h, coords_b.to(DEV), r).cpu()
    _assert_close(out_a, fc.forward64(*host, coords_a, r), fc.bound64(*host, coords_a, r), "run A (box passes)")
    _assert_close(out_b, fc.forward64(*host, coords_b, r), fc.bound64(*host, coords_b, r), "run B (per-query passes)")
    keep = ~moved
    assert int(keep.sum()) == g["h"] * g["w"] - 2 * segs
    same = out_a[:, :, keep] == out_b[:, :, keep]
    assert bool(same.all()), f"{int((~same).sum())} outputs of unmoved queries differ between the box and the per-query pass"
    assert bool((out_a[:, :, keep] != 0).any()) and not torch.equal(out_a[:, :, moved], out_b[:, :, moved])


def test_box_of_exactly_ktmax_targets_and_one_column_more():
    """Integer coordinates (level 0 is an exact gather). One interior segment's level-0 box is 12 x 32 = 384 = kTMax
    targets (nT = 24: every wave's six N-tiles, last LDS column 383) in the first input and 12 x 33 = 396 (per-query
    passes) in the second. Both match float64; the queries that were not shifted agree bit for bit."""
    r, f1h, f2h, host = _path_grid()
    g = fc.PATH_GRID
    dims = cc.level_dims(g["h"], g["w"], g["levels"])
    sy, sx = fc.KTMAX_SEGMENT
    outs = []
    for shift, kind, area in ((7, fc.BOX, 384), (8, fc.PER_QUERY, 396)):
        coords, touched = fc.ktmax_coords(shift)
        cen = fc.census(coords, r, dims)[0]
        assert (int(cen["kind"][0, sy, sx]), int(cen["area"][0, sy, sx])) == (kind, area)
        out = OPS.corr_lookup_otf(f1h, f2h, coords.to(DEV), r).cpu()
        _assert_close(out, fc.forward64(*host, coords, r), fc.bound64(*host, coords, r), f"box of {area} targets")
        outs.append(out)
    keep = ~touched
    same = outs[0][:, :, keep] == outs[1][:, :, keep]
    assert bool(same.all()), f"{int((~same).sum())} outputs of untouched queries differ across the kTMax edge"
    assert int(keep.sum()) == g["h"] * g["w"] - 2 and bool((outs[0][:, :, keep] != 0).any())


# ----------------------------------------------------------------------------------------------------------
# stray coordinates
# ----------------------------------------------------------------------------------------------------------
def test_stray_coordinates_give_zero_windows_and_leave_the_others_alone():
    """NaN, +-inf, 1e9 and +-2^22 * 2^l (refused at level l, accepted one level up, where it lies far outside) and their
    fp32 predecessors in a few queries of a smooth case: those queries' channels are exactly 0 at every level,
    everything is finite and matches float64, and every other query is bit-identical to the run where the stray
    queries hold their ordinary coordinates (a stray query does not move its segment's box)."""
    index = fc.CASE_IDS.index("r4-17x37-L4-C64-smooth")
    r, f1h, f2h, base, _, _ = _case(index)
    levels = len(f2h)
    coords, rows = cc.with_specials(base, levels)
    assert len(rows) == 4 + 4 * levels
    host = _host(f1h, f2h)
    ref, bound = fc.forward64(*host, coords, r), fc.bound64(*host, coords, r)
    assert bool((_rows(bound)[rows] == 0).all())
    got = OPS.corr_lookup_otf(f1h, f2h, coords.to(DEV), r).cpu()
    plain = OPS.corr_lookup_otf(f1h, f2h, base.to(DEV), r).cpu()
    assert bool(torch.isfinite(got).all())
    _assert_close(got, ref, bound, "stray coordinates")
    assert bool((_rows(got)[rows] == 0).all()) and bool((_rows(plain)[rows] != 0).any())
    others = torch.ones(_rows(got).shape[0], dtype=torch.bool)
    others[rows] = False
    assert torch.equal(_rows(got)[others], _rows(plain)[others])


# ----------------------------------------------------------------------------------------------------------
# the prepare step, bit for bit
# ----------------------------------------------------------------------------------------------------------
def _assert_same_bits(got, want, what):
    assert got.dtype == want.dtype == torch.float16 and got.shape == want.shape, (what, got.shape, want.shape)
    a, b = got.cpu().contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    assert torch.equal(a, b), (what, int((a != b).sum()), "fp16 bit patterns differ")


@pytest.mark.parametrize("index", range(len(fc.PREPARE_CASES)),
                         ids=[f"C{c}-{h}x{w}-B{b}-L{l}" for c, (h, w), b, l in fc.PREPARE_CASES])
def test_prepare_is_the_stated_arithmetic_bit_for_bit(index):
    """f1h = fp16_rne(fp32(fmap1 * (1.0f / sqrtf(C)))), f2h[l] = fp16_rne of the fp32 iterated floor 2x2 average pool."""
    c, (h, w), b, levels = fc.PREPARE_CASES[index]
    f1, f2 = fc.prepare_inputs(index)
    f1h, f2h = _prepared(f1, f2, levels)
    e1h, e2h = fc.prepare_exact(f1, f2, levels)
    assert len(f2h) == levels and [tuple(t.shape[1:3]) for t in f2h] == cc.level_dims(h, w, levels)
    _assert_same_bits(f1h, e1h, "f1h")
    for l in range(levels):
        _assert_same_bits(f2h[l], e2h[l], f"f2h[{l}]")


def test_prepare_rounds_planted_edge_values_once_and_to_even():
    """-0.0, fp16 subnormals and underflow, round-to-even ties, +-65504, +-65520 (inf) and ties that only the pooling
    forms: the sign of zero and every bit as include/oflow.h promises ("pooled in fp32 ... then rounded")."""
    _, _, _, levels = fc.PLANTED
    f1, f2 = fc.planted_inputs()
    f1h, f2h = _prepared(f1, f2, levels)
    e1h, e2h = fc.prepare_exact(f1, f2, levels)
    n = len(fc.planted_values())
    for name, got, want in (("fmap1", f1h[0, :, :, 5], e1h[0, :, :, 5]), ("fmap2", f2h[0][0, :, :, 3], e2h[0][0, :, :, 3])):
        a, b = got.reshape(-1)[:n].cpu(), want.reshape(-1)[:n]
        bad = [(v, float(x), float(y)) for v, x, y, eq in zip(fc.planted_values(), a, b, a.view(torch.int16) == b.view(torch.int16)) if not eq]
        assert not bad, (name, "(planted fmap2 value, stored, stated arithmetic)", bad)
    for ch in (7, 8, 9):
        for l in (1, 2):
            assert float(f2h[l][l, 0, 0, ch]) == float(e2h[l][l, 0, 0, ch]), (ch, l)
    _assert_same_bits(f1h, e1h, "f1h")
    for l in range(levels):
        _assert_same_bits(f2h[l], e2h[l], f"f2h[{l}]")


# ----------------------------------------------------------------------------------------------------------
# C ABI contracts (include/oflow.h), called directly
# ----------------------------------------------------------------------------------------------------------
def _carve(shape, dtype=torch.float32):
    """A NaN-filled buffer with GUARD elements in front of and behind a view of ``shape``."""
    n = 1
    for v in shape:
        n *= int(v)
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device=DEV)
    return buf, buf[GUARD : GUARD + n].view(*shape)


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _abi_lookup(f1h, f2h, coords, radius, out, c=None, levels=None, dims=None, null=()):
    b, _, h, w = coords.shape
    dims = [tuple(int(v) for v in t.shape[1:3]) for t in f2h] if dims is None else dims
    ptrs = (ctypes.c_void_p * _native.MAX_LEVELS)(*[None if f"f2h{l}" in null else t.data_ptr() for l, t in enumerate(f2h)])
    hs = (ctypes.c_int * _native.MAX_LEVELS)(*[d[0] for d in dims])
    ws = (ctypes.c_int * _native.MAX_LEVELS)(*[d[1] for d in dims])
    st = _native.load().oflow_corr_lookup_otf_f16(
        None if "f1h" in null else f1h.data_ptr(), None if "f2h" in null else ptrs, None if "level_h" in null else hs,
        None if "level_w" in null else ws, len(f2h) if levels is None else levels,
        None if "coords" in null else coords.data_ptr(), b, int(f1h.shape[3]) if c is None else c, h, w, radius,
        None if "out" in null else out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return st


def _abi_prepare(f1, f2, levels, f1h, f2h, scratch, c=None, null=()):
    b, ch, h, w = f1.shape
    ptrs = (ctypes.c_void_p * _native.MAX_LEVELS)(*[None if f"f2h{l}" in null else t.data_ptr() for l, t in enumerate(f2h)])
    st = _native.load().oflow_corr_otf_prepare_f16(
        None if "fmap1" in null else f1.data_ptr(), None if "fmap2" in null else f2.data_ptr(), b, ch if c is None else c,
        h, w, levels, None if "f1h" in null else f1h.data_ptr(), None if "f2h" in null else ptrs,
        None if "scratch" in null else scratch.data_ptr(), _stream())
    torch.cuda.synchronize()
    return st


def _abi_case():
    """Ragged in both directions: H = 5 (odd), W = 13 (no multiple of 16), B = 2."""
    index = fc.CASE_IDS.index("r4-5x13-L2-C32-mixed")
    r, f1h, f2h, coords, ref, bound = _case(index)
    assert coords.shape[0] == 2 and coords.shape[2] % 2 == 1 and coords.shape[3] % 16 != 0
    return r, f1h, f2h, coords.to(DEV), ref, bound


def test_abi_lookup_writes_every_element_and_nothing_else():
    """The output carved out of a NaN-filled buffer: every element is written, finite and equal to the op's result, the
    guards in front and behind stay NaN; the same with every window outside every level (the ``passes == 0`` fill)."""
    r, f1h, f2h, coords, ref, bound = _abi_case()
    b, _, h, w = coords.shape
    channels = len(f2h) * (2 * r + 1) ** 2
    for name, co in (("ordinary", coords), ("all outside", torch.full_like(coords, cc.FAR))):
        if name == "all outside":
            dims = [tuple(int(v) for v in t.shape[1:3]) for t in f2h]
            assert all(c[fc.BOX] == 0 and c[fc.PER_QUERY] == 0 for c in fc.census_counts(fc.census(co.cpu(), r, dims)))
        buf, out = _carve((b, channels, h, w))
        assert _abi_lookup(f1h, f2h, co, r, out) == 0, name
        assert bool(torch.isfinite(out).all()), (name, int((~torch.isfinite(out)).sum()), "elements not written")
        assert _guards_intact(buf), name
        assert torch.equal(out, OPS.corr_lookup_otf(f1h, f2h, co, r)), name
        if name == "ordinary":
            _assert_close(out, ref, bound, "C ABI lookup")
        else:
            assert bool((out == 0).all())


def test_abi_prepare_writes_every_element_and_nothing_else():
    """f1h, every f2h[l] and the scratch carved out of NaN-filled buffers (the scratch needs no initialisation): every
    element written, the fp16 tensors bit-identical to the stated arithmetic, the scratch holding the fp32 pooled levels
    1.. as (B*C, H_l, W_l) planes, all guards untouched."""
    c, (h, w), b, levels = 96, (9, 35), 2, 3
    f1, f2 = cc.gaussian(970, (b, c, h, w)), cc.gaussian(971, (b, c, h, w))
    dims = cc.level_dims(h, w, levels)
    buf1, f1h = _carve((b, h, w, c), torch.float16)
    carved = [_carve((b, hl, wl, c), torch.float16) for hl, wl in dims]
    bufs, scratch = _carve((b * c * sum(hl * wl for hl, wl in dims[1:]),))
    assert _abi_prepare(f1.to(DEV), f2.to(DEV), levels, f1h, [t for _, t in carved], scratch) == 0
    e1h, e2h = fc.prepare_exact(f1, f2, levels)
    _assert_same_bits(f1h, e1h, "f1h")
    assert _guards_intact(buf1)
    for l, (buf, t) in enumerate(carved):
        _assert_same_bits(t, e2h[l], f"f2h[{l}]")
        assert _guards_intact(buf), l
    assert _guards_intact(bufs) and bool(torch.isfinite(scratch).all())
    pooled, cur = [], f2
    for _ in range(1, levels):
        cur = F.avg_pool2d(cur, 2, stride=2)
        pooled.append(cur.reshape(-1))
    assert torch.equal(scratch.cpu(), torch.cat(pooled))


def test_abi_lookup_argument_errors_return_the_documented_codes():
    r, f1h, f2h, coords, _, _ = _abi_case()
    b, _, h, w = coords.shape
    dims = [tuple(int(v) for v in t.shape[1:3]) for t in f2h]
    for kwargs, radius, code in (
        ({"null": ("f1h",)}, r, E_NULL), ({"null": ("f2h",)}, r, E_NULL), ({"null": ("level_h",)}, r, E_NULL),
        ({"null": ("level_w",)}, r, E_NULL), ({"null": ("coords",)}, r, E_NULL), ({"null": ("out",)}, r, E_NULL),
        ({"null": ("f2h1",)}, r, E_NULL),
        ({"c": 40}, r, E_SHAPE), ({"c": 0}, r, E_SHAPE),
        ({"levels": 0}, r, E_LEVELS), ({"levels": 9}, r, E_LEVELS),
        ({}, 5, E_RADIUS), ({}, -1, E_RADIUS),
        ({"dims": [dims[0], (1, 6)]}, r, E_TINY), ({"dims": [dims[0], (2, 1)]}, r, E_TINY),
    ):
        buf, out = _carve((b, len(f2h) * (2 * r + 1) ** 2, h, w))
        st = _abi_lookup(f1h, f2h, coords, radius, out, **kwargs)
        assert st == code, (kwargs, radius, st)
        assert bool(torch.isnan(buf).all()), (kwargs, radius, "nothing may be enqueued")


def test_abi_prepare_argument_errors_return_the_documented_codes():
    c, (h, w), b, levels = 32, (5, 13), 2, 2
    f1, f2 = cc.gaussian(972, (b, c, h, w)).to(DEV), cc.gaussian(973, (b, c, h, w)).to(DEV)
    dims = cc.level_dims(h, w, levels)
    for kwargs, nl, code in (
        ({"null": ("fmap1",)}, levels, E_NULL), ({"null": ("fmap2",)}, levels, E_NULL), ({"null": ("f1h",)}, levels, E_NULL),
        ({"null": ("f2h",)}, levels, E_NULL), ({"null": ("f2h1",)}, levels, E_NULL),
        ({"null": ("scratch",)}, levels, E_NULL),  # a NULL scratch with more than one level
        ({"c": 40}, levels, E_SHAPE), ({}, 0, E_LEVELS), ({}, 9, E_LEVELS),
    ):
        buf1, f1h = _carve((b, h, w, c), torch.float16)
        carved = [_carve((b, hl, wl, c), torch.float16) for hl, wl in dims]
        bufs, scratch = _carve((b * c * dims[1][0] * dims[1][1],))
        st = _abi_prepare(f1, f2, nl, f1h, [t for _, t in carved], scratch, **kwargs)
        assert st == code, (kwargs, nl, st)
        for buf in [buf1, bufs] + [bf for bf, _ in carved]:
            assert bool(torch.isnan(buf).all()), (kwargs, nl, "nothing may be enqueued")
    # one level needs no scratch
    buf1, f1h = _carve((b, h, w, c), torch.float16)
    buf2, f2h0 = _carve((b, h, w, c), torch.float16)
    assert _abi_prepare(f1, f2, 1, f1h, [f2h0], None, null=("scratch",)) == 0
    assert bool(torch.isfinite(f1h).all()) and bool(torch.isfinite(f2h0).all()) and _guards_intact(buf1) and _guards_intact(buf2)


def test_a_level_of_one_pixel_is_prepared_but_refused_by_the_lookup():
    """2 x 2 pooled once is 1 x 1: the prepare step allows it (a pooled feature map is well defined), the lookup needs
    at least 2 pixels per side (OFLOW_E_TINY) and leaves its output alone."""
    c, b = 32, 2
    f1, f2 = cc.gaussian(974, (b, c, 2, 2)), cc.gaussian(975, (b, c, 2, 2))
    f1h, f2h = _prepared(f1, f2, 2)
    assert [tuple(t.shape[1:3]) for t in f2h] == [(2, 2), (1, 1)]
    e1h, e2h = fc.prepare_exact(f1, f2, 2)
    _assert_same_bits(f2h[1], e2h[1], "f2h[1]")
    coords = oc.grid_coords(b, 2, 2).to(DEV)
    buf, out = _carve((b, 2 * 9, 2, 2))
    assert _abi_lookup(f1h, f2h, coords, 1, out) == E_TINY and bool(torch.isnan(buf).all())
    buf, out = _carve((b, 9, 2, 2))
    assert _abi_lookup(f1h, f2h[:1], coords, 1, out) == 0 and bool(torch.isfinite(out).all()) and _guards_intact(buf)
    host = _host(f1h, f2h[:1])
    _assert_close(out, fc.forward64(*host, coords.cpu(), 1), fc.bound64(*host, coords.cpu(), 1), "2 x 2, one level")


def test_abi_two_calls_give_the_same_bits():
    r, f1h, f2h, coords, _, _ = _abi_case()
    b, _, h, w = coords.shape
    outs = []
    for _ in range(2):
        _, out = _carve((b, len(f2h) * (2 * r + 1) ** 2, h, w))
        assert _abi_lookup(f1h, f2h, coords, r, out) == 0
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
