"""The three kernels a training step differentiates through (csrc/corr_backward.hip) against float64, each on its own:
the lookup transpose per level and per radius, the floor-pool gradient fold, the feature-map gradient GEMMs at their
edge tiles, then the C ABI's documented contracts and the autograd wiring end to end. References and inputs:
tests/corr_backward_cases.py (checked on the CPU by tests/test_corr_backward_host.py).

Tolerances:
  * lookup transpose: |got - ref| <= 1e-6 * bound + 1e-30 per cell, bound = the transpose of |grad_out| = sum |w||g|.
    wx, wy are exact in fp32; 1 - w is one rounding, the weight product one, the multiply by g one, and at most three
    additions follow: <= 7 * 2^-24 = 4.2e-7 of the bound. Where the bound is 0 the output is exactly 0.
  * dyadic inputs (half-pixel / integer coordinates, integer gradients; level gradients k * 4^l): every product and
    sum is exact in fp32, so the output equals float64 bit for bit.
  * pool fold: <= 1e-6 * combine_bound (exact scales and products, at most 7 additions).
  * fmap gradients: 2e-5 * bound + 1e-6, the bar of test_fmap_gradient_gemms_match_fp64.
"""
from __future__ import annotations

import ctypes
import functools
import math

import pytest
import torch

import corr_backward_cases as cc
from model import CorrBlock, synthetic
from optical_flow import _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OPS = torch.ops.oflow
E_NULL = -1
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    _native.load()


def _lookup_bwd(g, coords, radius, h0, w0, levels):
    return [t.cpu() for t in OPS.corr_lookup_backward(g.to(DEV), coords.to(DEV), radius, h0, w0, levels)]


def _assert_levels_close(got, ref, bound, dims, q, what):
    """Per cell |got - ref| <= 1e-6 * bound + 1e-30, exactly 0 where the bound is 0."""
    assert len(got) == len(dims)
    dead = 0
    for l, (a, r_, bd) in enumerate(zip(got, ref, bound)):
        assert tuple(a.shape) == (q, 1) + tuple(dims[l]) and a.dtype == torch.float32, (what, l, a.shape)
        a = a.double()
        err = (a - r_).abs()
        live = bd > 0
        assert int(live.sum()) > 0, (what, l)
        dead += int((~live).sum())
        worst = float((err[live] / bd[live]).max())
        print(f"{what} level {l}: {int(live.sum())} live cells, worst |err| / bound = {worst:.3e}")
        assert bool((err <= 1e-6 * bd + 1e-30).all()), (what, l, worst)
        assert bool((a[~live] == 0).all()), (what, l, "a cell no window term reaches is not exactly 0")
    assert dead > 0, what  # both kinds of cell are present


# ----------------------------------------------------------------------------------------------------------
# lookup transpose: torch.ops.oflow.corr_lookup_backward
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,h0,w0,levels", cc.LOOKUP_CASES)
def test_lookup_backward_matches_fp64_per_level(radius, h0, w0, levels):
    """Every compiled radius, level sizes independent of the coords grid, coordinates inside / straddling / outside
    the levels with exact integers and negative fractions among them, Gaussian output gradient."""
    dims = cc.level_dims(h0, w0, levels)
    k = 2 * radius + 1
    coords = cc.mixed_coords(100 + 8 * levels + radius, cc.COORD_SHAPE, radius, h0, w0)
    b, _, h, w = coords.shape
    g = cc.gaussian(200 + radius, (b, levels * k * k, h, w))
    got = _lookup_bwd(g, coords, radius, h0, w0, levels)
    ref = cc.lookup_backward64(g, coords, radius, dims)
    bound = cc.lookup_backward_bound(g, coords, radius, dims)
    _assert_levels_close(got, ref, bound, dims, b * h * w, f"r={radius} {h0}x{w0}")


@pytest.mark.parametrize("radius,denom", [(4, 2), (0, 1), (7, 1)])
def test_lookup_backward_exact_on_dyadic_inputs(radius, denom):
    """Half-pixel (r = 4) or integer (r = 0, 7) coordinates and integer gradients in [-32, 32]: the weights are dyadic
    (<= 8 bits at level 3), every sum is exact in fp32, so each level equals float64 bit for bit -- the index mapping
    (window channel i*K + j <-> cell (x0 + i - r, y0 + j - r)) with no tolerance to hide in."""
    h0, w0, levels = 17, 37, 4
    dims = cc.level_dims(h0, w0, levels)
    k = 2 * radius + 1
    coords = cc.lattice_coords(31 + radius, cc.COORD_SHAPE, radius, h0, w0, denom)
    b, _, h, w = coords.shape
    g = cc.integers(32 + radius, (b, levels * k * k, h, w), 32)
    got = _lookup_bwd(g, coords, radius, h0, w0, levels)
    ref = cc.lookup_backward64(g, coords, radius, dims)
    for l, (a, r_) in enumerate(zip(got, ref)):
        assert int((r_ != 0).sum()) >= 30, (l, int((r_ != 0).sum()))
        assert torch.equal(a.double(), r_), (l, float((a.double() - r_).abs().max()))


@pytest.mark.parametrize("radius", [4, 3])
@pytest.mark.parametrize("layout", ["canonical", "tiled"])
def test_lookup_backward_is_the_adjoint_of_each_forward(layout, radius):
    """<fwd(P), G> = <P, bwd(G)> for the canonical and the tiled HIP lookup of the same pyramid: in float64 the two
    sides differ by <= 2e-6 * <|P|, bound> (each side is a set of <= 4-term sums, 1e-6 * bound each)."""
    b, c, h, w, levels = 2, 8, 9, 17, 3
    dims = cc.level_dims(h, w, levels)
    k = 2 * radius + 1
    f1, f2 = synthetic.synthetic_fmaps(b, c, h, w, stream=81)
    f1, f2 = f1.to(DEV), f2.to(DEV)
    coords = cc.mixed_coords(82 + radius, (b, 2, h, w), radius, h, w)
    g = cc.gaussian(83 + radius, (b, levels * k * k, h, w))
    pyr = list(OPS.corr_pyramid(f1, f2, levels))
    if layout == "canonical":
        out = OPS.corr_lookup(pyr, coords.to(DEV), radius)
    else:
        out = _native.corr_lookup_tiled(_native.corr_pyramid_tiled(f1, f2, levels), coords.to(DEV), radius)
    back = _lookup_bwd(g, coords, radius, h, w, levels)
    bound = cc.lookup_backward_bound(g, coords, radius, dims)
    lhs = float((out.cpu().double() * g.double()).sum())
    rhs = sum(float((p.cpu().double() * a.double()).sum()) for p, a in zip(pyr, back))
    scale = sum(float((p.cpu().double().abs() * bd).sum()) for p, bd in zip(pyr, bound))
    print(f"adjoint {layout} r={radius}: |lhs - rhs| = {abs(lhs - rhs):.3e}, <|P|, bound> = {scale:.3e}")
    assert scale > 0 and abs(lhs - rhs) <= 2e-6 * scale, (lhs, rhs, scale)


def test_lookup_backward_special_coordinates_give_zero_rows():
    """NaN, +-inf, 1e9, |c / 2^l| exactly 2^22 and the fp32 value just below it, as x or as y among ordinary
    coordinates: their rows are exactly zero at every level, and every other row is bit-identical to a run where the
    specials are replaced by a far-away finite value."""
    radius, h0, w0, levels = 4, 17, 37, 4
    dims = cc.level_dims(h0, w0, levels)
    base = cc.mixed_coords(5, cc.COORD_SHAPE, radius, h0, w0)
    coords, rows = cc.with_specials(base, levels)
    far, _ = cc.with_specials(base, levels, replace_by=cc.FAR)
    b, _, h, w = coords.shape
    g = cc.gaussian(6, (b, levels * 81, h, w))
    got = _lookup_bwd(g, coords, radius, h0, w0, levels)
    plain = _lookup_bwd(g, far, radius, h0, w0, levels)
    for l, (a, p) in enumerate(zip(got, plain)):
        assert bool(torch.isfinite(a).all()), l
        assert bool((a[rows] == 0).all()), l
        assert torch.equal(a, p), l
        assert bool((a != 0).any()), l
    ref = cc.lookup_backward64(g, coords, radius, dims)
    bound = cc.lookup_backward_bound(g, coords, radius, dims)
    _assert_levels_close(got, ref, bound, dims, b * h * w, "specials")


def test_lookup_backward_deterministic_on_dirty_memory():
    """Every (query, cell) is owned by one thread (no atomics) and every output cell is written or zero-filled: with
    the allocator's free blocks filled with NaN beforehand, three calls give finite, bit-identical levels."""
    radius, h0, w0, levels = 4, 17, 37, 4
    coords = cc.mixed_coords(9, cc.COORD_SHAPE, radius, h0, w0).to(DEV)
    b, _, h, w = coords.shape
    g = cc.gaussian(10, (b, levels * 81, h, w)).to(DEV)
    runs = []
    for _ in range(3):
        junk = [torch.full((1 << s,), NAN, device=DEV) for s in range(8, 23)]  # 1 KiB .. 16 MiB blocks of NaN
        del junk
        runs.append([t.clone() for t in OPS.corr_lookup_backward(g, coords, radius, h0, w0, levels)])
        torch.cuda.synchronize()
    for run in runs:
        for a, a0 in zip(run, runs[0]):
            assert bool(torch.isfinite(a).all())
            assert torch.equal(a, a0)


def test_lookup_backward_argument_errors():
    coords = cc.uniform_coords(1, cc.COORD_SHAPE, 1, 17, 37).to(DEV)
    b, _, h, w = coords.shape
    g = torch.zeros(b, 2 * 9, h, w, device=DEV)
    assert len(OPS.corr_lookup_backward(g, coords, 1, 17, 37, 2)) == 2
    with pytest.raises(RuntimeError, match="does not match"):
        OPS.corr_lookup_backward(g[:, :-1], coords, 1, 17, 37, 2)  # channel count
    with pytest.raises(RuntimeError, match="does not match"):
        OPS.corr_lookup_backward(g[..., :-1], coords, 1, 17, 37, 2)  # spatial size
    with pytest.raises(RuntimeError, match="levels"):
        OPS.corr_lookup_backward(g[:, :0], coords, 1, 17, 37, 0)
    with pytest.raises(RuntimeError, match="levels"):
        OPS.corr_lookup_backward(torch.zeros(b, 9, h, w, device=DEV), coords, 0, 17, 37, 9)
    with pytest.raises(RuntimeError, match="radius"):
        OPS.corr_lookup_backward(torch.zeros(b, 2 * 17 * 17, h, w, device=DEV), coords, 8, 17, 37, 2)
    # a level under 2 px: the exception type the forward lookup raises for OFLOW_E_TINY
    with pytest.raises(Exception) as fwd:
        OPS.corr_lookup([torch.zeros(b * h * w, 1, 3, 37, device=DEV), torch.zeros(b * h * w, 1, 1, 18, device=DEV)],
                        coords, 1)
    assert fwd.type is ValueError
    with pytest.raises(fwd.type, match="2 pixels"):
        OPS.corr_lookup_backward(g, coords, 1, 3, 37, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OPS.corr_lookup_backward(g.cpu(), coords.cpu(), 1, 17, 37, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OPS.corr_lookup_backward(g, coords.cpu(), 1, 17, 37, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OPS.corr_lookup_backward(g.cpu(), coords, 1, 17, 37, 2)
    for shape in ((0, 2, h, w), (b, 2, 0, w)):  # b*h*w = 0: empty-query gradients of the right shapes
        out = OPS.corr_lookup_backward(torch.zeros(shape[0], 18, shape[2], shape[3], device=DEV),
                                       torch.zeros(shape, device=DEV), 1, 17, 37, 2)
        assert [tuple(t.shape) for t in out] == [(0, 1, 17, 37), (0, 1, 8, 18)]
        assert all(t.dtype == torch.float32 and t.device.type == "cuda" for t in out)


# ----------------------------------------------------------------------------------------------------------
# C ABI contracts (include/oflow.h), called directly
# ----------------------------------------------------------------------------------------------------------
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _ptrs(tensors):
    return (ctypes.c_void_p * _native.MAX_LEVELS)(*[t.data_ptr() for t in tensors])


def _ints(values):
    return (ctypes.c_int * _native.MAX_LEVELS)(*values)


def _abi_lookup_backward(g, coords, radius, bufs, dims):
    b, _, h, w = coords.shape
    st = _native.load().oflow_corr_lookup_backward_f32(g.data_ptr(), coords.data_ptr(), b, h, w, radius, _ptrs(bufs),
                                                       _ints([d[0] for d in dims]), _ints([d[1] for d in dims]),
                                                       len(dims), _stream())
    torch.cuda.synchronize()
    return st


@functools.lru_cache(maxsize=None)
def _dyadic_lookup_case():
    radius, h0, w0, levels = 4, 17, 37, 4
    dims = cc.level_dims(h0, w0, levels)
    coords = cc.lattice_coords(41, cc.COORD_SHAPE, radius, h0, w0, 2)
    b, _, h, w = coords.shape
    g = cc.integers(42, (b, levels * 81, h, w), 32)
    return radius, dims, coords, g, cc.lookup_backward64(g, coords, radius, dims), b * h * w


def test_abi_lookup_backward_accumulates():
    """The header's '+=': two calls into the same zeroed buffers give exactly twice one call (dyadic inputs)."""
    radius, dims, coords, g, ref, q = _dyadic_lookup_case()
    gd, cd = g.to(DEV), coords.to(DEV)
    bufs = [torch.zeros(q, hl, wl, device=DEV) for hl, wl in dims]
    assert _abi_lookup_backward(gd, cd, radius, bufs, dims) == 0
    once = [t.cpu().clone() for t in bufs]
    assert _abi_lookup_backward(gd, cd, radius, bufs, dims) == 0
    for l, (a, t, r_) in enumerate(zip(once, bufs, ref)):
        assert torch.equal(a.double(), r_.reshape(a.shape)), l
        assert bool((a != 0).any()), l
        assert torch.equal(t.cpu(), 2 * a), l


def test_abi_lookup_backward_keeps_untouched_cells():
    """Pre-filled buffers: cells no window touches keep their value, the others hold value + gradient (exact)."""
    radius, dims, coords, g, ref, q = _dyadic_lookup_case()
    bound = cc.lookup_backward_bound(g, coords, radius, dims)
    fill = [cc.integers(43 + l, (q, hl, wl), 8) + 0.5 for l, (hl, wl) in enumerate(dims)]
    bufs = [f.to(DEV) for f in fill]
    assert _abi_lookup_backward(g.to(DEV), coords.to(DEV), radius, bufs, dims) == 0
    for l, (t, f, r_, bd) in enumerate(zip(bufs, fill, ref, bound)):
        t, dead = t.cpu(), bd.reshape(f.shape) == 0
        assert int(dead.sum()) > 0
        assert torch.equal(t[dead], f[dead]), l
        assert torch.equal(t.double(), f.double() + r_.reshape(f.shape)), l


def _guarded_levels(values):
    """The level tensors as slices of one allocation, with NaN rows after each: a read past a level's last row (the
    floor-pooled row or column an odd size drops) meets NaN instead of a neighbour."""
    q = values[0].shape[0]
    sizes = [v[0].numel() for v in values]
    slack = [2 * v.shape[-1] + 2 for v in values]
    store = torch.full((sum(q * n + s for n, s in zip(sizes, slack)),), NAN, device=DEV)
    views, off = [], 0
    for v, n, s in zip(values, sizes, slack):
        views.append(store[off : off + q * n].view(v.shape))
        views[-1].copy_(v)
        off += q * n + s
    return store, views


def _abi_combine(values, dims):
    store, views = _guarded_levels(values)
    st = _native.load().oflow_corr_pyramid_grad_combine_f32(_ptrs(views), _ints([d[0] for d in dims]),
                                                            _ints([d[1] for d in dims]), len(dims),
                                                            int(values[0].shape[0]), _stream())
    torch.cuda.synchronize()
    assert st == 0
    return [v.cpu() for v in views]


@pytest.mark.parametrize("hw,levels", cc.COMBINE_CASES)
def test_abi_pyramid_grad_combine_exact_and_fp64(hw, levels):
    dims = cc.level_dims(hw[0], hw[1], levels)
    q = cc.COMBINE_Q
    # level-l inputs k * 4^l, |k| <= 8: every term is a small integer, level 0 equals combine64 bit for bit
    ints = [cc.integers(50 + l, (q, 1, hl, wl), 8) * float(4**l) for l, (hl, wl) in enumerate(dims)]
    out = _abi_combine(ints, dims)
    assert torch.equal(out[0].double(), cc.combine64(ints, dims))
    for l in range(1, levels):
        assert torch.equal(out[l], ints[l]), l  # levels >= 1 are inputs only
    gauss = [cc.gaussian(60 + l, (q, 1, hl, wl)) for l, (hl, wl) in enumerate(dims)]
    out = _abi_combine(gauss, dims)
    err = (out[0].double() - cc.combine64(gauss, dims)).abs()
    bound = cc.combine_bound(gauss, dims)
    print(f"combine {hw} L={levels}: worst |err| / bound = {float((err / bound).max()):.3e}")
    assert bool((err <= 1e-6 * bound).all())
    for l in range(1, levels):
        assert torch.equal(out[l], gauss[l]), l


@pytest.mark.parametrize("hw,levels", [c for c in cc.COMBINE_CASES if c[1] > 1])
def test_abi_pyramid_grad_combine_drops_what_floor_pooling_dropped(hw, levels):
    """Level-0 cells in the last row or column that an odd level's floor pool dropped receive nothing from that level:
    with only level l non-zero (all ones), level 0 becomes 4^-l exactly on {(y, x): (y >> l, x >> l) inside level l}
    and stays 0 elsewhere."""
    dims = cc.level_dims(hw[0], hw[1], levels)
    q = cc.COMBINE_Q
    y, x = torch.arange(hw[0]), torch.arange(hw[1])
    for l in range(1, levels):
        vals = [torch.zeros(q, 1, hl, wl) for hl, wl in dims]
        vals[l].fill_(1.0)
        out = _abi_combine(vals, dims)[0]
        inside = ((y >> l) < dims[l][0])[:, None] & ((x >> l) < dims[l][1])[None, :]
        expect = inside.float() * (0.25**l)
        assert torch.equal(out, expect.expand(q, 1, hw[0], hw[1])), (l, dims[l])
        if hw[0] % 2:
            assert bool((out[:, :, -1, :] == 0).all()), (l, "last row of an odd height")
        if hw[1] % 2:
            assert bool((out[:, :, :, -1] == 0).all()), (l, "last column of an odd width")


def test_abi_fmap_grad_null_outputs():
    """Either output may be NULL: the other is bit-identical to the both-outputs call; both NULL is OFLOW_E_NULL;
    N = 0 is OK and launches nothing."""
    lib = _native.load()
    fn = lib.oflow_corr_fmap_grad_f32
    b, c, n = 2, 70, 130
    f1, f2 = cc.gaussian(71, (b, c, n)).to(DEV), cc.gaussian(72, (b, c, n)).to(DEV)
    g0 = cc.gaussian(73, (b, n, n)).to(DEV)
    s = 1.0 / math.sqrt(c)

    def call(want1, want2, n_=n):
        o1, o2 = torch.full((b, c, n), NAN, device=DEV), torch.full((b, c, n), NAN, device=DEV)
        st = fn(f1.data_ptr(), f2.data_ptr(), g0.data_ptr(), b, c, n_, s, o1.data_ptr() if want1 else None,
                o2.data_ptr() if want2 else None, _stream())
        torch.cuda.synchronize()
        return st, o1.cpu(), o2.cpu()

    st, both1, both2 = call(True, True)
    assert st == 0 and bool(torch.isfinite(both1).all()) and bool(torch.isfinite(both2).all())
    _assert_fmap_grads(both1.reshape(b, c, 1, n), both2.reshape(b, c, 1, n), g0.cpu().double(), g0.cpu().double().abs(),
                       f1.cpu().reshape(b, c, 1, n), f2.cpu().reshape(b, c, 1, n), "C ABI, both outputs")
    st, only1, none2 = call(True, False)
    assert st == 0 and torch.equal(only1, both1) and bool(torch.isnan(none2).all())
    st, none1, only2 = call(False, True)
    assert st == 0 and torch.equal(only2, both2) and bool(torch.isnan(none1).all())
    st, none1, none2 = call(False, False)
    assert st == E_NULL and bool(torch.isnan(none1).all()) and bool(torch.isnan(none2).all())
    st, none1, none2 = call(True, True, 0)
    assert st == 0 and bool(torch.isnan(none1).all()) and bool(torch.isnan(none2).all())


# ----------------------------------------------------------------------------------------------------------
# torch.ops.oflow.corr_pyramid_backward
# ----------------------------------------------------------------------------------------------------------
def _assert_fmap_grads(got1, got2, g0_ref, g0_bound, f1, f2, what):
    """Both fmap gradients vs the float64 GEMMs of g0_ref, to 2e-5 * bound + 1e-6 (bound: the GEMMs of |f|, g0_bound)."""
    b, c = f1.shape[:2]
    r1, r2 = cc.fmap_grads64(g0_ref, f1, f2)
    b1, b2 = cc.fmap_grads64(g0_bound, f1.abs(), f2.abs())
    for name, got, ref, bound in (("grad_f1", got1, r1, b1), ("grad_f2", got2, r2, b2)):
        assert got.shape == f1.shape and got.dtype == f1.dtype, (what, name)
        err = (got.cpu().double().reshape(b, c, -1) - ref).abs()
        tol = 2e-5 * bound + 1e-6
        print(f"{what} {name}: max |err| = {float(err.max()):.3e}, worst err / tol = {float((err / tol).max()):.3e}")
        assert bool((err <= tol).all()), (what, name, float((err / tol).max()))
        assert float(ref.abs().max()) > 0


@pytest.mark.parametrize("b,c,n", cc.GEMM_EDGE_CASES)
def test_pyramid_backward_gemm_edge_tiles_match_fp64(b, c, n):
    """N or C under one 64-tile, N under one 16-deep K chunk, exactly one tile, just past one and two tiles."""
    f1, f2 = cc.gaussian(c + n, (b, c, 1, n)), cc.gaussian(c + n + 1, (b, c, 1, n))
    g0 = cc.gaussian(c + n + 2, (b * n, 1, 1, n))
    g1, g2 = OPS.corr_pyramid_backward([g0.to(DEV)], f1.to(DEV), f2.to(DEV))
    _assert_fmap_grads(g1, g2, g0.double(), g0.double().abs(), f1, f2, f"gemm b={b} c={c} n={n}")


@functools.lru_cache(maxsize=None)
def _multi_level_case():
    b, c, h, w, levels = 2, 24, 17, 19, 4
    dims = cc.level_dims(h, w, levels)
    f1, f2 = cc.gaussian(91, (b, c, h, w)), cc.gaussian(92, (b, c, h, w))
    grads = [cc.gaussian(93 + l, (b * h * w, 1, hl, wl)) for l, (hl, wl) in enumerate(dims)]
    return f1, f2, grads, dims


def test_pyramid_backward_multi_level_matches_fp64():
    """Odd 17x19 level 0 under three floor pools: combine64 then the float64 GEMMs; bound from combine_bound."""
    f1, f2, grads, dims = _multi_level_case()
    g1, g2 = OPS.corr_pyramid_backward([g.to(DEV) for g in grads], f1.to(DEV), f2.to(DEV))
    _assert_fmap_grads(g1, g2, cc.combine64(grads, dims), cc.combine_bound(grads, dims), f1, f2, "multi-level")


def test_pyramid_backward_leaves_its_level0_gradient_unchanged():
    """The pool fold accumulates into level 0 in place -- into the op's own copy, never the caller's tensor."""
    f1, f2, grads, dims = _multi_level_case()
    dev = [g.to(DEV) for g in grads]
    keep = [g.clone() for g in dev]
    g1, _ = OPS.corr_pyramid_backward(dev, f1.to(DEV), f2.to(DEV))
    torch.cuda.synchronize()
    assert bool((g1 != 0).any())
    for l, (a, k) in enumerate(zip(dev, keep)):
        assert torch.equal(a, k), f"level {l} gradient was modified"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_pyramid_backward_low_precision_fmaps(dtype):
    """fp16 / bf16 feature maps: gradients of the fmaps' dtype, equal to the fp32 call on the same values rounded."""
    f1, f2, grads, dims = _multi_level_case()
    dev = [g.to(DEV) for g in grads]
    l1, l2 = f1.to(DEV).to(dtype), f2.to(DEV).to(dtype)
    g1, g2 = OPS.corr_pyramid_backward(dev, l1, l2)
    r1, r2 = OPS.corr_pyramid_backward(dev, l1.float(), l2.float())
    assert g1.dtype == dtype and g2.dtype == dtype and r1.dtype == torch.float32
    assert g1.shape == f1.shape and g2.shape == f2.shape
    assert torch.equal(g1, r1.to(dtype)) and torch.equal(g2, r2.to(dtype))
    _assert_fmap_grads(r1, r2, cc.combine64(grads, dims), cc.combine_bound(grads, dims), l1.float().cpu(),
                       l2.float().cpu(), f"fp32 call on {dtype} values")


# ----------------------------------------------------------------------------------------------------------
# autograd wiring, end to end
# ----------------------------------------------------------------------------------------------------------
def _wiring_inputs(radius, levels, hw, c, sigma, lookups=2):
    b, (h, w) = 2, hw
    k = 2 * radius + 1
    seed = 1000 * radius + 10 * levels + int(sigma)
    f1, f2 = cc.gaussian(seed + 1, (b, c, h, w)), cc.gaussian(seed + 2, (b, c, h, w))
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    grid = torch.stack((xs, ys), dim=0).float()[None].repeat(b, 1, 1, 1)
    cs = [grid + sigma * cc.gaussian(seed + 3 + i, (b, 2, h, w)) for i in range(lookups)]
    rs = [cc.gaussian(seed + 5 + i, (b, levels * k * k, h, w)) for i in range(lookups)]
    return f1, f2, cs, rs


def _assert_against_restatement(d1, d2, f1, f2, loss64, bound_levels, dims, what):
    """GPU fmap gradients vs float64 autograd of the restatement's loss, tolerance from the chain on absolute values."""
    a1, a2 = f1.double().requires_grad_(), f2.double().requires_grad_()
    loss64(a1, a2).backward()
    b, c = f1.shape[:2]
    g0_bound = cc.combine_bound(bound_levels, dims)
    b1, b2 = cc.fmap_grads64(g0_bound, f1.abs(), f2.abs())
    for name, got, ref, bound in (("grad_f1", d1.grad, a1.grad, b1), ("grad_f2", d2.grad, a2.grad, b2)):
        assert got is not None and got.shape == f1.shape and got.dtype == torch.float32, (what, name)
        err = (got.cpu().double() - ref).abs().reshape(b, c, -1)
        tol = 2e-5 * bound + 1e-6
        print(f"{what} {name}: max |err| = {float(err.max()):.3e}, worst err / tol = {float((err / tol).max()):.3e}")
        assert bool((err <= tol).all()), (what, name, float((err / tol).max()))
        assert float(ref.abs().max()) > 0


@pytest.mark.parametrize("sigma", [0.0, 3.0])
@pytest.mark.parametrize("radius,levels,hw,c", cc.WIRING_CASES)
def test_corrblock_gradients_match_fp64_restatement(radius, levels, hw, c, sigma):
    """CorrBlock under autograd with two lookups vs float64 matmul / sqrt(C), avg_pool2d, lookup64 (corr.py:38-87)."""
    f1, f2, cs, rs = _wiring_inputs(radius, levels, hw, c, sigma)
    dims = cc.level_dims(hw[0], hw[1], levels)
    d1, d2 = f1.to(DEV).requires_grad_(), f2.to(DEV).requires_grad_()
    cb = CorrBlock(d1, d2, num_levels=levels, radius=radius)
    sum((cb(co.to(DEV)) * r.to(DEV)).sum() for co, r in zip(cs, rs)).backward()

    def loss64(a1, a2):
        pyr = cc.corr_levels64(a1, a2, levels)
        return sum((cc.lookup64(pyr, co, radius) * r.double()).sum() for co, r in zip(cs, rs))

    per_lookup = [cc.lookup_backward_bound(r, co, radius, dims) for co, r in zip(cs, rs)]
    bound_levels = [sum(bl[l] for bl in per_lookup) for l in range(levels)]
    _assert_against_restatement(d1, d2, f1, f2, loss64, bound_levels, dims, f"r={radius} L={levels} {hw} s={sigma}")


def test_corrblock_gradient_of_one_level_only():
    """A loss on corr_pyramid[2] alone: levels 0, 1, 3 reach the backward as None and are taken as zeros."""
    radius, levels, hw, c = 3, 4, (17, 19), 24
    f1, f2, _, _ = _wiring_inputs(radius, levels, hw, c, 0.0)
    dims = cc.level_dims(hw[0], hw[1], levels)
    r = cc.gaussian(7, (2 * hw[0] * hw[1], 1) + dims[2])
    d1, d2 = f1.to(DEV).requires_grad_(), f2.to(DEV).requires_grad_()
    cb = CorrBlock(d1, d2, num_levels=levels, radius=radius)
    (cb.corr_pyramid[2] * r.to(DEV)).sum().backward()
    bound_levels = [torch.zeros(r.shape[0], 1, hl, wl, dtype=torch.float64) for hl, wl in dims]
    bound_levels[2] = r.double().abs()
    _assert_against_restatement(d1, d2, f1, f2, lambda a1, a2: (cc.corr_levels64(a1, a2, levels)[2] * r.double()).sum(),
                                bound_levels, dims, "level 2 only")


def test_corrblock_gradient_of_one_lookup_only():
    radius, levels, hw, c = 3, 3, (17, 19), 24
    f1, f2, cs, rs = _wiring_inputs(radius, levels, hw, c, 3.0)
    dims = cc.level_dims(hw[0], hw[1], levels)
    d1, d2 = f1.to(DEV).requires_grad_(), f2.to(DEV).requires_grad_()
    cb = CorrBlock(d1, d2, num_levels=levels, radius=radius)
    unused = cb(cs[0].to(DEV))
    (cb(cs[1].to(DEV)) * rs[1].to(DEV)).sum().backward()
    assert unused.requires_grad
    _assert_against_restatement(
        d1, d2, f1, f2,
        lambda a1, a2: (cc.lookup64(cc.corr_levels64(a1, a2, levels), cs[1], radius) * rs[1].double()).sum(),
        cc.lookup_backward_bound(rs[1], cs[1], radius, dims), dims, "second lookup only")


def test_lookup_under_autograd_refuses_levels_that_are_not_floor_pools():
    """The native transpose rebuilds the level sizes from level 0: other sizes raise in the forward."""
    b, h, w = 1, 9, 14
    q = b * h * w
    coords = cc.uniform_coords(2, (b, 2, h, w), 1, h, w).to(DEV)
    lv0 = torch.zeros(q, 1, 9, 14, device=DEV, requires_grad=True)
    lv1 = torch.zeros(q, 1, 4, 7, device=DEV, requires_grad=True)
    assert _native.corr_lookup([lv0, lv1], coords, 1).requires_grad
    with pytest.raises(RuntimeError, match="floor 2x2 pools"):
        _native.corr_lookup([lv1, lv0], coords, 1)  # swapped
    with pytest.raises(RuntimeError, match="floor 2x2 pools"):
        _native.corr_lookup([lv0, torch.zeros(q, 1, 5, 7, device=DEV, requires_grad=True)], coords, 1)  # ceil size
    with torch.no_grad():  # without a graph the sizes are the caller's business, as in the reference
        assert _native.corr_lookup([lv1, lv0], coords, 1).shape == (b, 18, h, w)
