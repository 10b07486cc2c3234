"""Pins the float64 restatements of tests/conv_s32_cases.py against the reference's own modules on the CPU, so that
the GPU tests built on them (test_gpu_conv_s32_tiles.py, test_gpu_update_fused.py) compare the kernels with the
operation the model defines and not with a second opinion of it: the plain convolution against nn.Conv2d, the
SepConvGRU half-step against SepConvGRU._step (update.py:91-97) in both kernel orientations and widths, the hoisted
form against the full form, and the three FusedUpdate elementwise operations against the op sequence of
update.py:69-161 (bias + activation after a bias-free convolution, merged z|r convolution, reset, blend, the mask
head's x0.25). Everything in float64, agreement to 1e-12 (reassociation of ~400-term float64 sums of O(1) values)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_s32_cases as cc
from model.update import BasicUpdateBlock, SepConvGRU

TOL = 1e-12


def _gru_module(ch, xc, ws1, bs1, kernel):
    """SepConvGRU in float64 whose first (1x5) or second (5x1) half carries the given weights."""
    gru = SepConvGRU(hidden_dim=ch, input_dim=ch + xc).double()
    tag = "1" if kernel == (1, 5) else "2"
    with torch.no_grad():
        for name, w, b in zip("zrq", ws1, bs1):
            conv = getattr(gru, f"conv{name}{tag}")
            assert tuple(conv.weight.shape) == tuple(w.shape)
            conv.weight.copy_(w.double())
            conv.bias.copy_(b.double())
    return gru, tag


@pytest.mark.parametrize("kh,kw", cc.KERNELS)
def test_conv_ref_is_the_module_convolution(kh, kw):
    x, wt, bias = cc.epi0_operands(kh, kw, 40, 6, (2, 5, 7), seed=kh * 10 + kw)
    conv = nn.Conv2d(40, 6, (kh, kw), padding=(kh // 2, kw // 2)).double()
    with torch.no_grad():
        conv.weight.copy_(wt.double())
        conv.bias.copy_(bias.double())
        ref = conv(x.double())
    y, bound = cc.conv_ref(x, wt, bias, kh, kw)
    assert y.dtype == torch.float64 and float((y - ref).abs().max()) <= TOL
    # the bound is the absolute-product sum: it dominates the bias-free result, with equality for same-signed operands
    assert bool(((y - bias.double().view(1, -1, 1, 1)).abs() <= bound * (1 + 1e-12)).all())
    ya, ba = cc.conv_ref(x.abs(), wt.abs(), None, kh, kw)
    assert float((ya - ba).abs().max()) <= TOL
    tol = cc.conv_tol(bound, y)
    assert torch.equal(tol, 2e-6 * bound + 1e-6 + 2.0 ** -22 * y.abs())


@pytest.mark.parametrize("ch,xc", [(128, 128), (64, 32), (128, 96)])
@pytest.mark.parametrize("kernel", [(1, 5), (5, 1)])
def test_gru_half_matches_sepconvgru_step(kernel, ch, xc):
    """gru_half_full = SepConvGRU._step; gru_half_hoisted with the context addend = gru_half_full."""
    h, inp, x, ws, bs = cc.gru_operands(*kernel, ch, xc, (2, 6, 9), seed=ch + xc + kernel[0])
    gru, tag = _gru_module(ch, xc, ws, bs, kernel)
    xin = torch.cat([inp, x], dim=1)
    with torch.no_grad():
        ref = gru._step(h.double(), xin.double(), *(getattr(gru, f"conv{n}{tag}") for n in "zrq"))
    full = cc.gru_half_full(h, xin, *ws, *bs)
    assert float((full.h - ref).abs().max()) <= TOL
    assert float((full.rh - full.r * h.double()).abs().max()) == 0.0
    add = cc.gru_context_addend(inp, *ws, *bs, ch)
    assert tuple(add.shape) == (2, 3 * ch, 6, 9)
    wsel = [cc.hoist_split(w, ch)[0] for w in ws]
    assert all(tuple(w.shape) == (ch, ch + xc, *kernel) for w in wsel)
    hoisted = cc.gru_half_hoisted(h, x, add, *wsel)
    for name in cc.GruHalf._fields:
        err = float((getattr(hoisted, name) - getattr(full, name)).abs().max())
        assert err <= TOL, (name, err)
    # the whole two-half GRU through the restatement = the module's forward
    h2, inp2, x2, ws2, bs2 = cc.gru_operands(5, 1, ch, xc, (2, 6, 9), seed=99)
    if kernel == (1, 5):
        _gru_module(ch, xc, ws2, bs2, (5, 1))  # (shape check only)
        with torch.no_grad():
            for name, w, b in zip("zrq", ws2, bs2):
                getattr(gru, f"conv{name}2").weight.copy_(w.double())
                getattr(gru, f"conv{name}2").bias.copy_(b.double())
            ref2 = gru(h.double(), xin.double())
        got2 = cc.gru_half_full(full.h, xin, *ws2, *bs2).h
        assert float((got2 - ref2).abs().max()) <= TOL


def test_gru_half_overrides_feed_the_second_launch():
    """rh / z given: the candidate and the blend use them (what a kernel stored between its two launches)."""
    h, inp, x, ws, bs = cc.gru_operands(1, 5, 64, 32, (1, 4, 6), seed=5)
    xin = torch.cat([inp, x], dim=1)
    base = cc.gru_half_full(h, xin, *ws, *bs)
    same = cc.gru_half_full(h, xin, *ws, *bs, rh=base.rh, z=base.z)
    assert torch.equal(same.h, base.h) and torch.equal(same.pre_q, base.pre_q)
    ones = cc.gru_half_full(h, xin, *ws, *bs, z=torch.ones_like(base.z))
    assert torch.equal(ones.h, base.q)
    zero = cc.gru_half_full(h, xin, *ws, *bs, rh=torch.zeros_like(base.rh))
    assert float((zero.pre_q - base.pre_q).abs().max()) > 1e-3
    none = cc.gru_half_hoisted(h, x, None, *[cc.hoist_split(w, 64)[0] for w in ws])
    hx = torch.cat([h, x], dim=1).double()
    assert torch.equal(none.pre_z, F.conv2d(hx, cc.hoist_split(ws[0], 64)[0].double(), padding=(0, 2)))


def test_fused_ops_restate_the_update_block():
    """bias_act_ref / gru_reset_ref / gru_blend_ref composed as FusedUpdate.step composes the kernels (bias-free
    convolutions, merged z|r weights) = BasicUpdateBlock's GRU, flow-head ReLU and 0.25 * mask in float64."""
    block = BasicUpdateBlock(corr_levels=1, corr_radius=1, hidden_dim=128).double()
    g = cc.gen(3)
    with torch.no_grad():
        for p in block.parameters():
            p.copy_(torch.randn(p.shape, generator=g).double() * 0.05)
    b, hh, ww = 2, 5, 7
    net = torch.tanh(torch.randn(b, 128, hh, ww, generator=g)).double()
    x = torch.randn(b, 256, hh, ww, generator=g).double()
    gru = block.gru
    with torch.no_grad():
        ref_net = gru(net, x)
        ref_mask = 0.25 * block.mask(ref_net)
        ref_hidden = F.relu(block.flow_head.conv1(ref_net))
        h = net
        for tag, pad in (("1", (0, 2)), ("2", (2, 0))):
            cz, cr, cq = (getattr(gru, f"conv{n}{tag}") for n in "zrq")
            hx = torch.cat([h, x], dim=1)
            zr = F.conv2d(hx, torch.cat([cz.weight, cr.weight]), None, padding=pad)
            rh = cc.gru_reset_ref(zr, cr.bias, h)
            q = F.conv2d(torch.cat([rh, x], dim=1), cq.weight, None, padding=pad)
            h = cc.gru_blend_ref(zr, cz.bias, q, cq.bias, h)
        assert float((h - ref_net).abs().max()) <= TOL
        m = cc.bias_act_ref(F.conv2d(h, block.mask[0].weight, None, padding=1), block.mask[0].bias, "relu", 1.0)
        mask = cc.bias_act_ref(F.conv2d(m, block.mask[2].weight, None), block.mask[2].bias, "none", 0.25)
        assert float((mask - ref_mask).abs().max()) <= TOL
        hid = cc.bias_act_ref(F.conv2d(h, block.flow_head.conv1.weight, None, padding=1), block.flow_head.conv1.bias,
                              "relu", 1.0)
        assert float((hid - ref_hidden).abs().max()) <= TOL


@pytest.mark.parametrize("act", ["none", "relu", "sigmoid", "tanh"])
def test_bias_act_ref_forms(act):
    g = cc.gen(7)
    x = torch.randn(3, 5, 11, generator=g) * 3
    bias = torch.randn(5, generator=g)
    ref = cc.bias_act_ref(x, bias, act, 0.25)
    want = {"none": lambda v: v, "relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act](
        x.double() + bias.double().view(1, 5, 1)) * 0.25
    assert ref.dtype == torch.float64 and float((ref - want).abs().max()) <= 1e-15
    f32 = cc.bias_act_ref(x, bias, act, 0.25, dtype=torch.float32)
    assert f32.dtype == torch.float32 and float((f32.double() - ref).abs().max()) <= 1e-6
    assert torch.equal(cc.bias_act_ref(x, None, act, 1.0), cc.act64(x.double(), act))
    # the fp32 forms of the two GRU operations track float64 the same way
    zr, q, h = torch.randn(2, 10, 9, generator=g), torch.randn(2, 5, 9, generator=g), torch.randn(2, 5, 9, generator=g)
    for fn, args in ((cc.gru_reset_ref, (zr, bias, h)), (cc.gru_blend_ref, (zr, bias, q, bias, h))):
        assert float((fn(*args, dtype=torch.float32).double() - fn(*args)).abs().max()) <= 1e-6


def test_leaf_tables():
    """decode_leaf inverts the hook's packing; the leaf lists hold what launch_bn / dispatch_conv instantiate."""
    leaf = cc.Leaf(5, 1, 128, 1, 4, 2, 4, 0, 1, 1)
    packed = (5 | 1 << 4 | 128 << 8 | 1 << 16 | 4 << 20 | 2 << 24 | 4 << 28 | 0 << 32 | 1 << 36 | 1 << 40)
    assert cc.decode_leaf(packed) == leaf == cc.expected_leaf(5, 1, 2, "breg128")
    assert cc.decode_leaf(0) == cc.Leaf(*([0] * 10))
    assert [len(cc.epi0_leaves(*k)) for k in cc.KERNELS] == [5, 8, 6, 6]
    assert set(cc.LEAVES) == set(cc.LEAF_BLOCK_N)
    for name, (bn, wm, wn, ty, breg, bd) in cc.LEAVES.items():
        assert wm * wn == 4 and bn % (32 * wn) == 0 and (bd == 1) == bool(breg)
        assert cc.LEAF_BLOCK_N[name] == bn
    groups = {(-(-cin // 32)) for _, cin, _ in cc.EPI0_CASES}
    assert groups == {1, 11, 12}
    assert {n for _, _, n in cc.EPI0_CASES} == {2, 126, 384}
    assert {ch for _, ch, _ in cc.GRU_CASES} == {64, 128}
