"""The float64 references of the correlation-backward GPU tests (tests/corr_backward_cases.py) checked on the CPU
against float64 autograd of the reference composition (oracle/corr.py: grid_sample behind bilinear_sampler, chained
avg_pool2d), so the GPU tests compare the kernels with something that is itself pinned down. No GPU needed."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

import corr_backward_cases as cc
from oracle import corr as ocorr


def _reference_lookup64(levels, coords, radius):
    """oracle/corr.py:corr_lookup on float64 levels: the same window deltas, bilinear_sampler (normalised grid)."""
    r = radius
    b, _, h1, w1 = coords.shape
    cent = coords.double().permute(0, 2, 3, 1).reshape(b * h1 * w1, 1, 1, 2)
    d = torch.linspace(-r, r, 2 * r + 1, dtype=torch.float64)
    dy, dx = torch.meshgrid(d, d, indexing="ij")
    delta = torch.stack((dy, dx), dim=-1).view(1, 2 * r + 1, 2 * r + 1, 2)
    outs = []
    for i, lvl in enumerate(levels):
        outs.append(ocorr.bilinear_sampler(lvl, cent / 2**i + delta).view(b, h1, w1, -1))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("radius,levels,hw", cc.HOST_CASES)
def test_lookup_backward64_equals_autograd_of_the_reference_composition(radius, levels, hw):
    dims = cc.level_dims(hw[0], hw[1], levels)
    k = 2 * radius + 1
    coords = cc.mixed_coords(300 + radius, cc.COORD_SHAPE, radius, hw[0], hw[1])
    b, _, h, w = coords.shape
    g = cc.gaussian(40 + radius, (b, levels * k * k, h, w))
    got = cc.lookup_backward64(g, coords, radius, dims)
    lv = [torch.zeros(b * h * w, 1, hl, wl, dtype=torch.float64, requires_grad=True) for hl, wl in dims]
    ref = torch.autograd.grad(_reference_lookup64(lv, coords, radius), lv, g.double())
    nonzero = 0
    for l, (a, r_) in enumerate(zip(got, ref)):
        assert a.shape == r_.shape == (b * h * w, 1) + dims[l]
        err = float((a - r_).abs().max())
        assert err <= 1e-12, (l, err)
        nonzero += int((r_ != 0).sum())
    assert nonzero > 0
    # the forward itself, on random levels
    pyr = [cc.gaussian(50 + l, (b * h * w, 1, hl, wl)).double() for l, (hl, wl) in enumerate(dims)]
    fwd = float((cc.lookup64(pyr, coords, radius) - _reference_lookup64(pyr, coords, radius)).abs().max())
    assert fwd <= 1e-12, fwd
    # the bound is the transpose of |g|: it dominates the gradient and vanishes only where the gradient does
    bound = cc.lookup_backward_bound(g, coords, radius, dims)
    for a, bd in zip(got, bound):
        assert bool((a.abs() <= bd * (1 + 1e-12)).all())
        assert bool((a[bd == 0] == 0).all())


def test_lookup64_matches_the_oracle_loop_restatement():
    """lookup64 against oracle/corr.py:corr_lookup_f64 (the per-query loop), which the forward tests trust."""
    radius, dims = 2, cc.level_dims(9, 14, 3)
    coords = cc.mixed_coords(77, (1, 2, 4, 9), radius, 9, 14)
    pyr = [cc.gaussian(60 + l, (36, 1, hl, wl)).double() for l, (hl, wl) in enumerate(dims)]
    ref = ocorr.corr_lookup_f64([p.numpy() for p in pyr], coords.numpy(), radius)
    assert float((cc.lookup64(pyr, coords, radius) - torch.from_numpy(ref)).abs().max()) <= 1e-12


@pytest.mark.parametrize("hw,levels", cc.COMBINE_CASES + [((16, 32), 4), ((7, 9), 3)])
def test_combine64_equals_autograd_of_chained_avg_pool(hw, levels):
    dims = cc.level_dims(hw[0], hw[1], levels)
    q = cc.COMBINE_Q
    grads = [cc.gaussian(70 + l, (q, 1, hl, wl)).double() for l, (hl, wl) in enumerate(dims)]
    x = torch.zeros(q, 1, hw[0], hw[1], dtype=torch.float64, requires_grad=True)
    pyr, lvl = [x], x
    for hl, wl in dims[1:]:
        lvl = F.avg_pool2d(lvl, 2, stride=2)
        assert tuple(lvl.shape[-2:]) == (hl, wl)
        pyr.append(lvl)
    loss = sum((p * g).sum() for p, g in zip(pyr, grads))
    (ref,) = torch.autograd.grad(loss, x)
    got = cc.combine64(grads, dims)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12
    assert bool((got.abs() <= cc.combine_bound(grads, dims) * (1 + 1e-12)).all())


def test_special_coordinates_give_exactly_zero_rows():
    radius, levels, hw = 4, 4, (17, 37)
    dims = cc.level_dims(hw[0], hw[1], levels)
    base = cc.mixed_coords(5, cc.COORD_SHAPE, radius, hw[0], hw[1])
    coords, rows = cc.with_specials(base, levels)
    assert len(rows) == 4 + 4 * levels
    b, _, h, w = coords.shape
    g = cc.gaussian(6, (b, levels * 81, h, w))
    got = cc.lookup_backward64(g, coords, radius, dims)
    far, _ = cc.with_specials(base, levels, replace_by=cc.FAR)
    ref = cc.lookup_backward64(g, far, radius, dims)
    for a, r_ in zip(got, ref):
        assert bool(torch.isfinite(a).all())
        assert bool((a[rows] == 0).all())
        assert torch.equal(a, r_)  # every other row as if the special were merely far away
    assert any(bool((a != 0).any()) for a in got)
    out = cc.lookup64([torch.ones(b * h * w, 1, hl, wl, dtype=torch.float64) for hl, wl in dims], coords, radius)
    assert bool((out.permute(0, 2, 3, 1).reshape(b * h * w, -1)[rows] == 0).all())


def test_fmap_chain_equals_autograd_of_the_restatement():
    """combine64 + fmap_grads64 of the lookup transposes = float64 autograd through corr_levels64 + lookup64."""
    radius, levels, (h, w), c = 1, 3, (9, 10), 5
    f1, f2 = cc.gaussian(1, (2, c, h, w)).double(), cc.gaussian(2, (2, c, h, w)).double()
    coords = cc.mixed_coords(3, (2, 2, h, w), radius, h, w)
    r = cc.gaussian(4, (2, levels * 9, h, w)).double()
    a1, a2 = f1.clone().requires_grad_(), f2.clone().requires_grad_()
    (cc.lookup64(cc.corr_levels64(a1, a2, levels), coords, radius) * r).sum().backward()
    dims = cc.level_dims(h, w, levels)
    g1, g2 = cc.fmap_grads64(cc.combine64(cc.lookup_backward64(r, coords, radius, dims), dims), f1, f2)
    assert float((g1 - a1.grad.reshape(2, c, -1)).abs().max()) <= 1e-12
    assert float((g2 - a2.grad.reshape(2, c, -1)).abs().max()) <= 1e-12
