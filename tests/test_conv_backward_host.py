"""The float64 closed form, bounds and tolerance constant of the convolution backward tests
(tests/conv_backward_cases.py) checked on the CPU against autograd of ``F.conv2d``, so the GPU tests compare the kernels
with something that is itself pinned down; then the ABI and operator layers as far as they go without a GPU (exported
symbols, the workspace query, registration, Meta kernels, autograd wiring, the CPU refusal) and the model's routing
attribute. No GPU needed."""
from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import conv_backward_cases as cc
from model import RAFT
from model import update as upd
from optical_flow import _native, _ops

META = torch.device("meta")
E_NULL, E_SHAPE = -1, -2  # include/oflow.h: OFLOW_E_NULL, OFLOW_E_SHAPE
NEW_SYMBOLS = ("oflow_conv2d_backward_input_f32", "oflow_conv2d_backward_weight_f32",
               "oflow_conv2d_backward_weight_workspace_floats", "oflow_conv2d_backward_weight_slab_pixels")


def _autograd(case: cc.Case, dtype):
    x, w = case.x.clone().to(dtype).requires_grad_(), case.weight.clone().to(dtype).requires_grad_()  # (copies)
    b = torch.zeros(w.shape[0], dtype=dtype, requires_grad=True)
    kh, kw = w.shape[-2:]
    F.conv2d(x, w, b, padding=(kh // 2, kw // 2)).backward(case.grad_out.to(dtype))
    return x.grad, w.grad, b.grad


# ------------------------------------------------------------------------------------------------- the references
def test_cases_cover_the_kernels_edges():
    lib = _native.load()
    assert lib.oflow_conv2d_backward_weight_slab_pixels() == cc.SLAB  # the K-split cases are built around this
    assert len(set(cc.CASE_IDS)) == len(cc.CASES)
    dims = [c.dims for c in cc.CASES]
    assert {(d[5], d[6]) for d in dims} >= {(1, 1), (3, 3), (1, 5), (5, 1), (7, 7)}
    assert {d[2] for d in dims} >= {2, 33, 126, 324} and {d[1] for d in dims} >= {2, 33, 126, 576}
    assert {(d[3], d[4], d[5], d[6]) for d in dims} >= {(1, 1, 1, 1), (1, 70, 1, 5), (70, 1, 5, 1), (5, 9, 7, 7)}
    pixels = {d[0] * d[3] * d[4] for d in dims if d[0] > 1}  # several images: a pixel tile spans two of them
    assert pixels >= {cc.PIXEL_TILE - 1, cc.PIXEL_TILE, cc.PIXEL_TILE + 1, cc.K_CHUNK + 1}
    nslabs = {cc.slabs(c): c for c in cc.CASES}
    one = [c for c in cc.CASES if c.dims[0] * c.dims[3] * c.dims[4] == cc.SLAB]
    assert one and cc.slabs(one[0]) == 1  # exactly one full slab
    many = cc.BY_NAME["3x3-c8-n8-3x41x37"]
    b, _, _, h, w, _, _ = many.dims
    assert cc.slabs(many) == 3 and b * h * w > 2 * cc.SLAB and (b * h * w) % cc.SLAB and 2 in nslabs
    assert cc.BY_NAME["1x5-c384-n128-2x6x40"].dims == (2, 128, 384, 6, 40, 1, 5)
    again = cc.make_case(cc.SHAPES[7])
    assert all(torch.equal(a, b) for a, b in zip(again[1:], cc.CASES[7][1:])) and again.name == cc.CASES[7].name
    single = cc.CASES[-1]
    assert int((single.grad_out != 0).sum()) == single.dims[1]  # every output channel of one pixel


@pytest.mark.parametrize("case", cc.CASES, ids=cc.CASE_IDS)
def test_closed_form_equals_fp64_autograd(case):
    refs = _autograd(case, torch.float64)
    got = cc.backward64(*case[1:])
    bounds = cc.bounds64(*case[1:])
    for r, g, bd in zip(refs, got, bounds):
        assert g.shape == r.shape and g.dtype == torch.float64
        scale = float(bd.max())
        assert scale > 0 and float((g - r).abs().max()) <= 1e-13 * scale
        assert bool((g.abs() <= bd * (1 + 1e-12)).all()) and bool((g[bd == 0] == 0).all())
    assert float(refs[0].abs().max()) > 0 and float(refs[1].abs().max()) > 0


def test_taps_outside_a_1x1_image_contribute_nothing():
    """(2, 33, 1, 1) under a 3x3 kernel: only the centre tap is inside, so dx = gy . w[:, :, 1, 1] and dw is zero
    off the centre."""
    case = cc.BY_NAME["3x3-c33-n2-2x1x1"]
    dx, dw, db = cc.backward64(*case[1:])
    want = case.grad_out.double()[:, :, 0, 0] @ case.weight.double()[:, :, 1, 1]
    assert torch.allclose(dx[:, :, 0, 0], want, rtol=1e-13, atol=0)
    off = torch.ones(3, 3, dtype=torch.bool)
    off[1, 1] = False
    assert bool((dw[:, :, off] == 0).all()) and bool((dw[:, :, 1, 1] != 0).all())
    assert torch.equal(db, case.grad_out.double().sum(dim=(0, 2, 3)))


def test_single_pixel_gradient_has_exact_zeros():
    case = cc.CASES[-1]
    _, _, bounds = cc.reference(case)
    assert float((bounds[0] == 0).double().mean()) > 0.5  # most of dx is outside the 3x3 footprint of the one pixel


def test_reference_fp32_autograd_calibrates_the_tolerance():
    """The calibration of K: ATen's own fp32 autograd of F.conv2d on the CPU needs at most K / 4 (in units of
    U * bound) on every committed case and gradient (K = 4 x that maximum, rounded up: the device sums in another
    order)."""
    worst = [0.0, 0.0, 0.0]
    for case in cc.CASES:
        grads = _autograd(case, torch.float32)
        r = cc.error_ratios(*grads, case)
        print(f"{case.name}: fp32 reference needs {r[0]:.3f} (dx), {r[1]:.3f} (dw), {r[2]:.3f} (db) U bound")
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"maxima: dx {worst[0]:.3f}, dw {worst[1]:.3f}, db {worst[2]:.3f} (K / 4 = {cc.K / 4})")
    assert max(worst) <= cc.K / 4
    assert max(worst) >= cc.K / 8  # and the constant is not looser than measured
    for case in cc.CASES:  # the same statement through the assertion the GPU tests use
        cc.assert_close(*_autograd(case, torch.float32), case, "fp32 reference")


def test_tolerance_catches_one_misplaced_term():
    """What K is for: on the longest sum (4551 pixels) dropping a single average-sized term of an element's sum is
    outside the tolerance, while (n + 2) U bound alone would let it pass."""
    case = cc.BY_NAME["3x3-c8-n8-3x41x37"]
    (_, dw, _), (_, tol, _), (_, bound, _) = cc.reference(case)
    n = cc.term_counts(case)[1]
    term = bound / n  # the mean magnitude of one term
    assert bool((term > tol).all())
    assert bool((term < (n + 2) * cc.U * bound).all())
    bad = (dw + term).float()
    with pytest.raises(AssertionError):
        cc.assert_close(None, bad, None, case, "one term too many")


# ------------------------------------------------------------------------------------------------- ABI, no launch
def test_library_exports_and_binds_the_new_symbols():
    lib = ctypes.CDLL(_native.library_path())
    bound = _native.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _native.SYMBOLS
        assert getattr(bound, name).argtypes is not None
    assert bound.oflow_conv2d_backward_weight_workspace_floats.restype is ctypes.c_longlong


def test_workspace_query():
    lib = _native.load()
    q = lib.oflow_conv2d_backward_weight_workspace_floats
    for case in cc.CASES:
        b, cout, cin, h, w, kh, kw = case.dims
        assert q(*case.dims) == cc.slabs(case) * (cout * cin * kh * kw + cout)
    assert q(8, 128, 384, 46, 62, 1, 5) == 12 * (128 * 384 * 5 + 128)
    for bad in ((0, 8, 8, 4, 4, 3, 3), (1, 8, 8, 4, 4, 2, 3), (1, 8, 8, 4, 4, 3, 9), (1, 8, 8, 4, 4, 3, -1),
                (1, 65536, 8, 4, 4, 3, 3), (65536, 8, 8, 2048, 1, 3, 3)):
        assert q(*bad) == 0


def test_argument_errors_are_reported_without_launch():
    """Status codes need no GPU: they are returned before anything is enqueued (the pointers are never dereferenced on
    the host)."""
    lib = _native.load()
    p = 4096  # any non-null address
    good = (1, 8, 8, 4, 4, 3, 3)
    assert lib.oflow_conv2d_backward_input_f32(None, p, *good, p, None) == E_NULL
    assert lib.oflow_conv2d_backward_input_f32(p, None, *good, p, None) == E_NULL
    assert lib.oflow_conv2d_backward_input_f32(p, p, *good, None, None) == E_NULL
    assert lib.oflow_conv2d_backward_weight_f32(None, p, *good, p, p, p, None) == E_NULL
    assert lib.oflow_conv2d_backward_weight_f32(p, None, *good, p, p, p, None) == E_NULL  # dw needs x
    assert lib.oflow_conv2d_backward_weight_f32(p, p, *good, None, None, p, None) == E_NULL  # no output
    assert lib.oflow_conv2d_backward_weight_f32(p, p, *good, p, p, None, None) == E_NULL  # no workspace
    for bad in ((0, 8, 8, 4, 4, 3, 3), (1, 0, 8, 4, 4, 3, 3), (1, 8, -1, 4, 4, 3, 3), (1, 8, 8, 0, 4, 3, 3),
                (1, 8, 8, 4, 0, 3, 3), (1, 8, 8, 4, 4, 2, 3), (1, 8, 8, 4, 4, 3, 4), (1, 8, 8, 4, 4, 9, 1),
                (1, 8, 8, 4, 4, 0, 1), (1, 65536, 8, 4, 4, 1, 1), (65536, 8, 8, 2048, 1, 1, 1),
                (1, 65535, 65535, 1, 1, 1, 1)):
        assert lib.oflow_conv2d_backward_input_f32(p, p, *bad, p, None) == E_SHAPE, bad
        assert lib.oflow_conv2d_backward_weight_f32(p, p, *bad, p, p, p, None) == E_SHAPE, bad


# ------------------------------------------------------------------------------------------------- operator layer
def test_ops_are_registered():
    _native.load()
    for name in ("conv2d_same", "conv2d_same_backward"):
        assert name in _ops.OPS
        assert getattr(torch.ops.oflow, name).default._schema.name == f"oflow::{name}"


def test_meta_shapes_and_argument_errors():
    _native.load()
    ops = torch.ops.oflow
    x, w, b = torch.empty(3, 33, 7, 9, device=META), torch.empty(5, 33, 1, 5, device=META), torch.empty(5, device=META)
    for bias in (b, None):
        out = ops.conv2d_same(x, w, bias)
        assert tuple(out.shape) == (3, 5, 7, 9) and out.dtype == torch.float32
    g = torch.empty(3, 5, 7, 9, device=META)
    for need in ([True, True, True], [True, False, False], [False, True, False], [False, False, True], [False] * 3):
        gx, gw, gb = ops.conv2d_same_backward(g, x, w, need)
        assert tuple(gx.shape) == (tuple(x.shape) if need[0] else (0,))
        assert tuple(gw.shape) == (tuple(w.shape) if need[1] else (0,))
        assert tuple(gb.shape) == ((5,) if need[2] else (0,))
    for bad_w in (torch.empty(5, 33, 2, 5, device=META), torch.empty(5, 33, 1, 9, device=META), torch.empty(5, 33, 4, 4, device=META)):
        with pytest.raises(RuntimeError, match="not supported"):
            ops.conv2d_same(x, bad_w, None)
        with pytest.raises(RuntimeError, match="not supported"):
            ops.conv2d_same_backward(g, x, bad_w, [True, True, True])
    with pytest.raises(RuntimeError, match=r"groups = 1"):
        ops.conv2d_same(x, torch.empty(5, 11, 1, 5, device=META), None)  # a grouped convolution's weight
    with pytest.raises(RuntimeError, match="float32"):
        ops.conv2d_same(x.half(), w.half(), None)
    with pytest.raises(RuntimeError, match="bias"):
        ops.conv2d_same(x, w, torch.empty(4, device=META))
    for bad_g in (g[:, :4], g[..., :-1], g[:2], g[0]):
        with pytest.raises(RuntimeError, match="grad_out"):
            ops.conv2d_same_backward(bad_g, x, w, [True, True, True])


def test_gradients_flow_on_meta_tensors():
    _native.load()
    x = torch.empty(2, 8, 5, 9, device=META, requires_grad=True)
    w = torch.empty(4, 8, 3, 3, device=META, requires_grad=True)
    b = torch.empty(4, device=META, requires_grad=True)
    out = torch.ops.oflow.conv2d_same(x, w, b)
    assert out.requires_grad
    out[..., 3:-2].sum().backward()  # a cropped, expanded gradient
    assert x.grad.shape == x.shape and w.grad.shape == w.shape and b.grad.shape == b.shape
    x2 = torch.empty(2, 8, 5, 9, device=META)  # an input that needs no gradient; no bias
    w2 = torch.empty(4, 8, 3, 3, device=META, requires_grad=True)
    torch.ops.oflow.conv2d_same(x2, w2, None).sum().backward()
    assert w2.grad.shape == w2.shape


def test_cpu_tensors_raise():
    _native.load()
    x, w, g = torch.zeros(1, 2, 3, 3), torch.zeros(2, 2, 3, 3), torch.zeros(1, 2, 3, 3)
    for call in (lambda: torch.ops.oflow.conv2d_same(x, w, None),
                 lambda: torch.ops.oflow.conv2d_same_backward(g, x, w, [True, True, False])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ------------------------------------------------------------------------------------------------- model routing
def test_conv_backward_impl_attribute():
    model = RAFT()
    assert model.conv_backward_impl == "aten" and model.update_block.conv_backward_impl == "aten"
    keys = set(model.state_dict())
    model.conv_backward_impl = "native"
    assert set(model.state_dict()) == keys  # a plain attribute: no parameter, buffer or key
    assert upd.CONV_BACKWARD_IMPLS == ("aten", "native")


def test_cpu_tensors_keep_calling_the_modules():
    """On the CPU (and without autograd) "native" changes nothing: conv_forward calls the module, bit for bit."""
    torch.manual_seed(0)
    block = upd.BasicUpdateBlock(corr_levels=4, corr_radius=4)
    net, inp = torch.randn(1, 128, 5, 6), torch.randn(1, 128, 5, 6)
    corr, flow = torch.randn(1, 324, 5, 6), torch.randn(1, 2, 5, 6)
    outs = {}
    for impl in ("aten", "native"):
        block.conv_backward_impl = impl
        outs[impl] = block(net, inp, corr, flow)
        assert block.gru.conv_backward_impl == block.encoder.conv_backward_impl == block.flow_head.conv_backward_impl == impl
    assert all(torch.equal(a, b) for a, b in zip(outs["aten"], outs["native"]))
    assert all("conv2d_same" not in str(t.grad_fn).lower() for t in outs["native"])
    block.conv_backward_impl = "miopen"
    with pytest.raises(ValueError, match="conv_backward_impl"):
        block(net, inp, corr, flow)
    conv = nn.Conv2d(2, 3, 3, padding=1)
    with pytest.raises(ValueError, match="conv_backward_impl"):
        upd.conv_forward(conv, flow, "triton")


def test_only_same_convolutions_are_routed():
    x = torch.empty(1, 4, 8, 8, device=META, requires_grad=True)
    ok = lambda conv: upd.native_backward_conv(conv.to(META), x)  # noqa: E731
    # (a meta tensor is not on the GPU: the geometry tests below are reached through a stand-in for is_cuda)
    assert not ok(nn.Conv2d(4, 4, 3, padding=1))

    class OnGpu(torch.Tensor):
        is_cuda = True

    xg = torch.empty(1, 4, 8, 8, requires_grad=True).as_subclass(OnGpu)
    ok = lambda conv: upd.native_backward_conv(conv, xg)  # noqa: E731
    assert ok(nn.Conv2d(4, 4, 3, padding=1)) and ok(nn.Conv2d(4, 4, (1, 5), padding=(0, 2))) and ok(nn.Conv2d(4, 4, 1))
    assert ok(nn.Conv2d(4, 4, 7, padding=3, bias=False))
    assert not ok(nn.Conv2d(4, 4, 3, padding=1, stride=2)) and not ok(nn.Conv2d(4, 4, 3, padding=0))
    assert not ok(nn.Conv2d(4, 4, 3, padding=2, dilation=2)) and not ok(nn.Conv2d(4, 4, 3, padding=1, groups=2))
    assert not ok(nn.Conv2d(4, 4, 9, padding=4)) and not ok(nn.Conv2d(4, 4, 2, padding=1))
    assert not ok(nn.Conv2d(4, 4, 3, padding=1, padding_mode="reflect")) and not ok(nn.Identity())
    with torch.no_grad():
        assert not ok(nn.Conv2d(4, 4, 3, padding=1))
    frozen = nn.Conv2d(4, 4, 3, padding=1).requires_grad_(False)
    assert not upd.native_backward_conv(frozen, torch.empty(1, 4, 8, 8).as_subclass(OnGpu))  # nothing to differentiate
