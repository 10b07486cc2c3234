"""The encoders' native backward against float64: the strided convolution backward (csrc/conv_backward.hip) and the
norm-layer backward (csrc/norm_backward.hip) through the C ABI, their null-output and shape contracts, the operators
under autograd (eager and torch.compile), then ``BasicEncoder`` and one RAFT training step with
``encoder_backward_impl = "native"`` against ``"aten"``. Closed forms, inputs and tolerances:
tests/encoder_backward_cases.py (checked and calibrated on the CPU by tests/test_encoder_backward_host.py).

Tolerances: convolution min(K_CONV, n + 2) * 2^-24 * bound per element, norm layers K_NORM * 2^-24 * bound, with bound
the closed form on absolute values and the constants four times what ATen's own fp32 autograd needs on the CPU.
"""
from __future__ import annotations

import ctypes

import pytest
import torch
import torch.nn.functional as F

import encoder_backward_cases as ec
from model import RAFT, synthetic
from model.extractor import BasicEncoder
from optical_flow import _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
OPS = torch.ops.oflow
E_NULL, E_SHAPE = -1, -2
NAN = float("nan")
MULTI_SLAB = "3x3-c8-n8-3x81x73-s2"
CONV_PICK = ("3x3-c33-n126-3x5x7-s2", "1x1-c33-n33-2x5x7-s2", "7x7-c3-n64-2x9x10-s2", MULTI_SLAB)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need a ROCm GPU"
    _native.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _ptr(t, keep=True):
    return t.data_ptr() if keep and t is not None else None


def _dirty_allocator():
    """Fill the allocator's free blocks with NaN: later outputs and workspaces land in them."""
    junk = [torch.full((1 << s,), NAN, device=DEV) for s in range(8, 22)]
    del junk


# ----------------------------------------------------------------------------------------------------------
# strided convolution: C ABI
# ----------------------------------------------------------------------------------------------------------
def _cdev(case):
    return case.grad_out.to(DEV), case.x.to(DEV), case.weight.to(DEV)


def _conv_buffers(case):
    n_ws = _native.load().oflow_conv2d_strided_backward_weight_workspace_floats(*case.dims)
    assert n_ws > 0
    return (torch.full(case.x.shape, NAN, device=DEV), torch.full(case.weight.shape, NAN, device=DEV),
            torch.full((case.dims[1],), NAN, device=DEV), torch.full((n_ws,), NAN, device=DEV))


def _abi_wgrad(case, g, x, want_w=True, want_b=True, dims=None, with_g=True, with_x=True, with_ws=True, generic=False):
    """oflow_conv2d_strided_backward_weight[_generic]_f32 on NaN-filled outputs and workspace -> (status, grad_weight,
    grad_bias, workspace)."""
    _, gw, gb, ws = _conv_buffers(case)
    lib = _native.load()
    fn = lib.oflow_conv2d_strided_backward_weight_generic_f32 if generic else lib.oflow_conv2d_strided_backward_weight_f32
    st = fn(_ptr(g, with_g), _ptr(x, with_x), *(dims or case.dims), _ptr(gw, want_w), _ptr(gb, want_b), _ptr(ws, with_ws),
            _stream())
    torch.cuda.synchronize()
    return st, gw.cpu(), gb.cpu(), ws.cpu()


def _abi_dgrad(case, g, w, dims=None, with_g=True, with_w=True, with_out=True):
    gx = _conv_buffers(case)[0]
    st = _native.load().oflow_conv2d_strided_backward_input_f32(_ptr(g, with_g), _ptr(w, with_w), *(dims or case.dims),
                                                                 _ptr(gx, with_out), _stream())
    torch.cuda.synchronize()
    return st, gx.cpu()


@pytest.mark.parametrize("case", ec.CONV_CASES, ids=ec.CONV_IDS)
def test_conv_abi_matches_fp64(case):
    """Every element of the three outputs is written (the buffers and the workspace start as NaN) and is within
    tolerance of float64; elements with a zero bound (absent parity classes, untouched pixels) are exactly 0."""
    g, x, w = _cdev(case)
    st, gx = _abi_dgrad(case, g, w)
    assert st == 0
    st, gw, gb, ws = _abi_wgrad(case, g, x)
    assert st == 0 and bool(torch.isfinite(ws).all())  # the whole queried workspace is used
    ec.assert_conv_close(gx, gw, gb, case, "C ABI")


@pytest.mark.parametrize("case", ec.STRIDE1_CASES, ids=ec.STRIDE1_IDS)
def test_conv_abi_stride_1_equals_the_stride_1_entry_points(case):
    lib = _native.load()
    g, x, w = _cdev(case)
    st, gx = _abi_dgrad(case, g, w)
    st2, gw, gb, _ = _abi_wgrad(case, g, x)
    assert st == 0 and st2 == 0
    ox, ow, ob, ws = _conv_buffers(case)
    d7 = case.dims[:7]
    assert lib.oflow_conv2d_backward_weight_workspace_floats(*d7) == ws.numel()
    assert lib.oflow_conv2d_backward_input_f32(g.data_ptr(), w.data_ptr(), *d7, ox.data_ptr(), _stream()) == 0
    assert lib.oflow_conv2d_backward_weight_f32(g.data_ptr(), x.data_ptr(), *d7, ow.data_ptr(), ob.data_ptr(), ws.data_ptr(),
                                                _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(gx, ox.cpu()) and torch.equal(gw, ow.cpu()) and torch.equal(gb, ob.cpu())
    ec.assert_conv_close(gx, gw, gb, case, "stride 1")


def test_conv_folded_weight_gradient_against_the_generic_path():
    """Cin <= 4 takes the folded (channel, tap) tiles; the same data zero-padded to 5 channels and the generic hook take
    the per-tap tiles: all within tolerance of float64. (Each element's fma chain runs over the same pixels in the same
    order on both paths, so the bits are expected to agree too; that is printed, the contract is the tolerance.)"""
    for name in ("7x7-c4-n33-2x9x10-s2", "7x7-c3-n64-2x16x24-s2"):
        case = ec.CONV_BY_NAME[name]
        g, x, w = _cdev(case)
        st, folded, fb, _ = _abi_wgrad(case, g, x)
        st2, generic, gb, _ = _abi_wgrad(case, g, x, generic=True)
        assert st == 0 and st2 == 0 and torch.equal(fb, gb)
        ec.assert_conv_close(None, folded, fb, case, "folded")
        ec.assert_conv_close(None, generic, gb, case, "generic hook")
        wide = ec.pad_channels(case, 5)
        st3, padded, pb, _ = _abi_wgrad(wide, g, wide.x.to(DEV))
        assert st3 == 0 and not bool(padded[:, case.dims[2]:].any())
        ec.assert_conv_close(None, padded[:, : case.dims[2]].contiguous(), pb, case, "padded to c5")
        print(f"{name}: folded == generic hook: {torch.equal(folded, generic)}, folded == padded c5: "
              f"{torch.equal(folded, padded[:, : case.dims[2]])}")


@pytest.mark.parametrize("name", [MULTI_SLAB, "7x7-c3-n64-2x9x10-s2"])
def test_conv_abi_forms_only_the_requested_outputs(name):
    case = ec.CONV_BY_NAME[name]
    g, x, w = _cdev(case)
    st, both_w, both_b, ws = _abi_wgrad(case, g, x)
    assert st == 0 and bool(torch.isfinite(ws).all())
    st, only_w, no_b, _ = _abi_wgrad(case, g, x, want_b=False)
    assert st == 0 and torch.equal(only_w, both_w) and bool(torch.isnan(no_b).all())
    for with_x in (True, False):
        st, no_w, only_b, _ = _abi_wgrad(case, g, x, want_w=False, with_x=with_x)
        assert st == 0 and torch.equal(only_b, both_b) and bool(torch.isnan(no_w).all())
    untouched = lambda r: all(bool(torch.isnan(t).all()) for t in r[1:])  # noqa: E731
    for kw in (dict(want_w=False, want_b=False), dict(with_g=False), dict(with_x=False), dict(with_ws=False)):
        r = _abi_wgrad(case, g, x, **kw)
        assert r[0] == E_NULL and untouched(r), kw
    for kw in (dict(with_g=False), dict(with_w=False)):
        r = _abi_dgrad(case, g, w, **kw)
        assert r[0] == E_NULL and untouched(r), kw
    assert _abi_dgrad(case, g, w, with_out=False)[0] == E_NULL


@pytest.mark.parametrize("dims", [(2, 126, 33, 4, 8, 3, 3, 0), (2, 126, 33, 4, 8, 3, 3, 3), (2, 126, 33, 4, 8, 3, 3, -2),
                                  (2, 126, 33, 4, 8, 2, 3, 2), (2, 126, 33, 4, 8, 3, 4, 2), (2, 126, 33, 4, 8, 9, 3, 2),
                                  (2, 126, 33, 4, 8, 3, 9, 2), (0, 126, 33, 4, 8, 3, 3, 2), (2, 0, 33, 4, 8, 3, 3, 2),
                                  (2, 126, 0, 4, 8, 3, 3, 2), (2, 126, 33, 0, 8, 3, 3, 2), (2, 126, 33, 4, -8, 3, 3, 2),
                                  (2, 65536, 33, 4, 8, 3, 3, 2), (65536, 126, 33, 4096, 2, 3, 3, 2)])
def test_conv_abi_bad_shapes_return_e_shape(dims):
    case = ec.CONV_BY_NAME["3x3-c33-n126-2x4x8-s2"]
    g, x, w = _cdev(case)
    st, gx = _abi_dgrad(case, g, w, dims=dims)
    assert st == E_SHAPE and bool(torch.isnan(gx).all())
    for generic in (False, True):
        st, gw, gb, ws = _abi_wgrad(case, g, x, dims=dims, generic=generic)
        assert st == E_SHAPE
        assert bool(torch.isnan(gw).all()) and bool(torch.isnan(gb).all()) and bool(torch.isnan(ws).all())


# ----------------------------------------------------------------------------------------------------------
# norm layers: C ABI
# ----------------------------------------------------------------------------------------------------------
def _bn_params(case):
    return tuple(t.to(DEV) for t in (case.weight, case.bias, case.running_mean, case.running_var))


def _abi_norm(case, want=(True, True, True), with_g=True, with_x=True, with_ws=True, shape=None, eps=ec.EPS):
    """The norm backward of ``case`` on NaN-filled outputs and workspace -> (status, (dx[, dgamma, dbeta]), workspace)."""
    lib = _native.load()
    g, x = case.grad_out.to(DEV), case.x.to(DEV)
    b, c, h, w = shape or case.x.shape
    dx = torch.full(case.x.shape, NAN, device=DEV)
    if case.kind == "instance":
        st = lib.oflow_instance_norm_backward_f32(_ptr(g, with_g), _ptr(x, with_x), b * c, h * w, eps, int(case.relu),
                                                  _ptr(dx, want[0]), _stream())
        torch.cuda.synchronize()
        return st, (dx.cpu(),), None
    n_ws = lib.oflow_frozen_batch_norm_backward_workspace_floats(case.x.shape[0], case.x.shape[1], _hw(case))
    assert n_ws == 2 * case.x.shape[0] * case.x.shape[1]
    dg, db = torch.full((case.x.shape[1],), NAN, device=DEV), torch.full((case.x.shape[1],), NAN, device=DEV)
    ws = torch.full((n_ws,), NAN, device=DEV)
    st = lib.oflow_frozen_batch_norm_backward_f32(_ptr(g, with_g), _ptr(x, with_x), *(t.data_ptr() for t in _bn_params(case)),
                                                  b, c, h * w, eps, int(case.relu), _ptr(dx, want[0]), _ptr(dg, want[1]),
                                                  _ptr(db, want[2]), _ptr(ws, with_ws), _stream())
    torch.cuda.synchronize()
    return st, (dx.cpu(), dg.cpu(), db.cpu()), ws.cpu()


def _hw(case):
    return case.x.shape[2] * case.x.shape[3]


@pytest.mark.parametrize("case", ec.NORM_CASES, ids=ec.NORM_IDS)
def test_norm_abi_matches_fp64(case):
    st, got, ws = _abi_norm(case)
    assert st == 0
    assert ws is None or bool(torch.isfinite(ws).all())  # the whole queried workspace is used
    ec.assert_norm_close(got, case, "C ABI")


def test_norm_abi_with_an_unaligned_base_pointer():
    """Tensors that start 4 bytes past a 16-byte boundary: the scalar path, the same values."""
    for name in ("instance-2x64x12x20-relu", "frozen_bn-2x64x12x20-relu"):
        case = ec.NORM_BY_NAME[name]
        lib = _native.load()
        n = case.x.numel()
        bufs = [torch.full((n + 1,), NAN, device=DEV) for _ in range(3)]
        g, x, dx = (b[1:] for b in bufs)
        g.copy_(case.grad_out.flatten()), x.copy_(case.x.flatten())
        assert x.data_ptr() % 16 == 4
        b, c, h, w = case.x.shape
        if case.kind == "instance":
            st = lib.oflow_instance_norm_backward_f32(g.data_ptr(), x.data_ptr(), b * c, h * w, ec.EPS, 1, dx.data_ptr(),
                                                      _stream())
        else:
            st = lib.oflow_frozen_batch_norm_backward_f32(g.data_ptr(), x.data_ptr(),
                                                          *(t.data_ptr() for t in _bn_params(case)), b, c, h * w, ec.EPS, 1,
                                                          dx.data_ptr(), None, None, None, _stream())
        torch.cuda.synchronize()
        assert st == 0 and bool(torch.isnan(bufs[2][0]))
        ec.assert_norm_close((dx.view(case.x.shape).cpu(),), case, "unaligned")
        if case.kind != "instance":  # (no statistics involved: the same bits as the float4 path)
            assert torch.equal(dx.view(case.x.shape).cpu(), _abi_norm(case)[1][0])


def test_norm_abi_null_and_shape_contracts():
    inst, bn = ec.NORM_BY_NAME["instance-2x3x5x7-relu"], ec.NORM_BY_NAME["frozen_bn-2x3x5x7-relu"]
    nan = lambda ts: all(bool(torch.isnan(t).all()) for t in ts)  # noqa: E731
    for kw in (dict(with_g=False), dict(with_x=False), dict(want=(False, True, True))):
        st, got, _ = _abi_norm(inst, **kw)
        assert st == E_NULL and nan(got), kw
    for kw in (dict(shape=(0, 3, 5, 7)), dict(shape=(2, 3, 0, 7)), dict(shape=(2, -3, 5, 7)), dict(eps=-1.0)):
        st, got, _ = _abi_norm(inst, **kw)
        assert st == E_SHAPE and nan(got), kw
    st, full, _ = _abi_norm(bn)
    assert st == 0
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)):
        st, got, ws = _abi_norm(bn, want=want)
        assert st == 0
        for n, t, f in zip(want, got, full):
            assert torch.equal(t, f) if n else bool(torch.isnan(t).all()), want
        assert bool(torch.isfinite(ws).all()) == (want[1] or want[2])
    st, got, ws = _abi_norm(bn, want=(True, False, False), with_ws=False)  # dx alone needs no workspace
    assert st == 0 and torch.equal(got[0], full[0])
    for kw in (dict(want=(False, False, False)), dict(with_g=False), dict(with_x=False), dict(with_ws=False)):
        st, got, ws = _abi_norm(bn, **kw)
        assert st == E_NULL and nan(got) and nan((ws,)), kw
    for kw in (dict(shape=(0, 3, 5, 7)), dict(shape=(2, 0, 5, 7)), dict(shape=(2, 3, 5, 0)), dict(eps=-1.0)):
        st, got, ws = _abi_norm(bn, **kw)
        assert st == E_SHAPE and nan(got) and nan((ws,)), kw


# ----------------------------------------------------------------------------------------------------------
# operators
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONV_PICK + ("3x3-c64-n96-2x12x20-s2",))
def test_conv_forward_is_bit_identical_to_conv2d(name):
    case = ec.CONV_BY_NAME[name]
    _, x, w = _cdev(case)
    kh, kw = w.shape[-2:]
    bias = ec.gaussian(7, (w.shape[0],)).to(DEV)
    for s in (2, 1):
        for b in (bias, None):
            want = F.conv2d(x, w, b, stride=s, padding=(kh // 2, kw // 2))
            with torch.no_grad():
                assert torch.equal(OPS.conv2d_strided(x, w, b, s), want)
            got = OPS.conv2d_strided(x.clone().requires_grad_(), w, b, s)
            assert got.requires_grad and torch.equal(got.detach(), want)


def _conv_op_grads(case, gout=None, bias=True):
    g, x, w = _cdev(case)
    x, w = x.requires_grad_(), w.requires_grad_()
    b = torch.zeros(w.shape[0], device=DEV, requires_grad=True) if bias else None
    OPS.conv2d_strided(x, w, b, case.stride).backward(g if gout is None else gout)
    return x.grad, w.grad, (b.grad if bias else None)


@pytest.mark.parametrize("case", ec.CONV_CASES, ids=ec.CONV_IDS)
def test_conv_autograd_matches_fp64(case):
    ec.assert_conv_close(*_conv_op_grads(case), case, "autograd")


def test_conv_autograd_with_a_noncontiguous_and_an_expanded_grad_out():
    case = ec.CONV_BY_NAME["3x3-c33-n126-3x5x7-s2"]
    g = case.grad_out.to(DEV)
    wide = torch.full((g.shape[0], g.shape[1], g.shape[2] + 5, g.shape[3] + 3), NAN, device=DEV)
    view = wide[:, :, 2 : 2 + g.shape[2], 1 : 1 + g.shape[3]]
    view.copy_(g)
    assert not view.is_contiguous()
    plain, cropped = _conv_op_grads(case), _conv_op_grads(case, gout=view)
    assert all(torch.equal(a, b) for a, b in zip(plain, cropped))
    _, x, w = _cdev(case)
    x, w, b = x.requires_grad_(), w.requires_grad_(), torch.zeros(w.shape[0], device=DEV, requires_grad=True)
    OPS.conv2d_strided(x, w, b, 2).sum().backward()  # a stride-0 expanded gradient
    ones = ec.ConvCase(case.name + "-ones", torch.ones_like(case.grad_out), case.x, case.weight, 2)
    ec.assert_conv_close(x.grad, w.grad, b.grad, ones, "expanded grad_out")


def test_conv_op_forms_only_the_wanted_gradients():
    case = ec.CONV_BY_NAME["3x3-c33-n126-3x5x7-s2"]
    g, x, w = _cdev(case)
    wr = w.clone().requires_grad_()
    OPS.conv2d_strided(x, wr, None, 2).backward(g)  # the stem's situation: the input needs no gradient
    ec.assert_conv_close(None, wr.grad, None, case, "weight only")
    full = OPS.conv2d_strided_backward(g, x, w, 2, [True, True, True])
    for need in ([True, False, False], [False, True, False], [False, False, True], [True, False, True], [False] * 3):
        got = OPS.conv2d_strided_backward(g, x, w, 2, need)
        for n, t, f in zip(need, got, full):
            assert t.numel() == (f.numel() if n else 0) and (not n or torch.equal(t, f))
    with pytest.raises(RuntimeError, match="grad_out"):
        OPS.conv2d_strided_backward(g, x, w, 1, [True, True, True])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OPS.conv2d_strided_backward(g.cpu(), x, w, 2, [True, True, True])
    with pytest.raises(RuntimeError, match="not supported"):
        OPS.conv2d_strided(x, torch.zeros(4, 33, 2, 2, device=DEV), None, 2)
    with pytest.raises(RuntimeError, match="stride"):
        OPS.conv2d_strided(x, w, None, 3)
    empty = OPS.conv2d_strided_backward(torch.zeros(0, 126, 3, 4, device=DEV), torch.zeros(0, 33, 5, 7, device=DEV), w, 2,
                                        [True] * 3)
    assert tuple(empty[0].shape) == (0, 33, 5, 7) and not bool(empty[1].any()) and not bool(empty[2].any())
    meta = OPS.conv2d_strided(x.to("meta"), w.to("meta"), None, 2)
    assert tuple(meta.shape) == tuple(g.shape)


def _module_norm(case):
    if case.kind == "instance":
        return torch.nn.InstanceNorm2d(case.x.shape[1]).to(DEV)
    m = torch.nn.BatchNorm2d(case.x.shape[1], eps=ec.EPS).to(DEV).eval()
    with torch.no_grad():
        for dst, src in zip((m.weight, m.bias, m.running_mean, m.running_var), _bn_params(case)):
            dst.copy_(src)
    return m


def _norm_op(case, x, params=None):
    if case.kind == "instance":
        return OPS.instance_norm_act(x, ec.EPS, case.relu)
    return OPS.frozen_batch_norm_act(x, *(params or _bn_params(case)), ec.EPS, case.relu)


@pytest.mark.parametrize("case", [c for c in ec.NORM_CASES if _hw(c) > 1], ids=[c.name for c in ec.NORM_CASES if _hw(c) > 1])
def test_norm_op_forward_equals_the_module_and_autograd_matches_fp64(case):
    """(Planes of one element: F.instance_norm refuses them; the C ABI test covers them.)"""
    mod = _module_norm(case)
    x = case.x.to(DEV)
    with torch.no_grad():
        want = mod(x)
        want = torch.relu_(want) if case.relu else want
        assert torch.equal(_norm_op(case, x), want)
    xr = x.clone().requires_grad_()
    params = tuple(t.clone().requires_grad_(i < 2) for i, t in enumerate(_bn_params(case))) if case.kind != "instance" else None
    out = _norm_op(case, xr, params)
    assert out.requires_grad and torch.equal(out.detach(), want)
    out.backward(case.grad_out.to(DEV))
    got = (xr.grad,) + ((params[0].grad, params[1].grad) if params else ())
    ec.assert_norm_close(got, case, "autograd")


def test_norm_ops_masks_views_empty_batches_and_refusals():
    bn = ec.NORM_BY_NAME["frozen_bn-2x3x5x7-relu"]
    g, x, p = bn.grad_out.to(DEV), bn.x.to(DEV), _bn_params(bn)
    full = OPS.frozen_batch_norm_act_backward(g, x, *p, ec.EPS, True, [True] * 3)
    ec.assert_norm_close(full, bn, "backward op")
    for need in ([True, False, False], [False, True, False], [False, False, True], [False, True, True], [False] * 3):
        got = OPS.frozen_batch_norm_act_backward(g, x, *p, ec.EPS, True, need)
        for n, t, f in zip(need, got, full):
            assert t.numel() == (f.numel() if n else 0) and (not n or torch.equal(t, f))
    wr = p[0].clone().requires_grad_()  # only the scale needs a gradient
    OPS.frozen_batch_norm_act(x, wr, *p[1:], ec.EPS, True).backward(g)
    assert torch.equal(wr.grad, full[1])
    for case in (bn, ec.NORM_BY_NAME["instance-2x3x5x7-relu"]):
        g, x = case.grad_out.to(DEV), case.x.to(DEV)
        wide = torch.full((2, 3, 9, 10), NAN, device=DEV)
        view = wide[:, :, 2:7, 1:8]
        view.copy_(g)
        grads = []
        for gout in (g, view):
            xr = x.clone().requires_grad_()
            _norm_op(case, xr).backward(gout)
            grads.append(xr.grad)
        assert torch.equal(*grads)
        xr = x.clone().requires_grad_()
        _norm_op(case, xr).sum().backward()  # a stride-0 expanded gradient
        ones = case._replace(name=case.name + "-ones", grad_out=torch.ones_like(case.grad_out))
        ec.assert_norm_close((xr.grad,), ones, "expanded grad_out")
    e = torch.zeros(0, 3, 5, 7, device=DEV)
    assert tuple(OPS.instance_norm_act_backward(e, e, ec.EPS, True).shape) == (0, 3, 5, 7)
    got = OPS.frozen_batch_norm_act_backward(e, e, *p, ec.EPS, True, [True] * 3)
    assert tuple(got[0].shape) == (0, 3, 5, 7) and not bool(got[1].any()) and not bool(got[2].any())
    with pytest.raises(RuntimeError, match="grad_out"):
        OPS.instance_norm_act_backward(g[..., :-1], x, ec.EPS, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OPS.instance_norm_act_backward(g.cpu(), x, ec.EPS, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OPS.frozen_batch_norm_act_backward(g.cpu(), x, *p, ec.EPS, True, [True] * 3)
    with pytest.raises(RuntimeError, match="running_var"):
        OPS.frozen_batch_norm_act(x, p[0], p[1], p[2], p[3][:-1], ec.EPS, True)
    xm = x.to("meta")
    assert tuple(OPS.instance_norm_act(xm, ec.EPS, True).shape) == tuple(x.shape)
    pm = tuple(t.to("meta") for t in p)
    assert [tuple(t.shape) for t in OPS.frozen_batch_norm_act_backward(xm, xm, *pm, ec.EPS, True, [True, False, True])] == [
        tuple(x.shape), (0,), (3,)]


def test_backwards_are_deterministic_on_dirty_memory():
    """No atomics and nothing left to the caller to zero: with the allocator's free blocks filled with NaN beforehand
    (the outputs and the workspaces land in them), two runs give finite, bit-identical gradients."""
    cg, cx, cw = _cdev(ec.CONV_BY_NAME[MULTI_SLAB])  # three slabs
    inst, bn = ec.NORM_BY_NAME["instance-2x64x12x20-relu"], ec.NORM_BY_NAME["frozen_bn-2x64x12x20-relu"]
    ig, ix = inst.grad_out.to(DEV), inst.x.to(DEV)
    bg, bx, bp = bn.grad_out.to(DEV), bn.x.to(DEV), _bn_params(bn)
    runs = []
    for _ in range(2):
        _dirty_allocator()
        out = [t.clone() for t in OPS.conv2d_strided_backward(cg, cx, cw, 2, [True, True, True])]
        _dirty_allocator()
        out.append(OPS.instance_norm_act_backward(ig, ix, ec.EPS, True).clone())
        _dirty_allocator()
        out += [t.clone() for t in OPS.frozen_batch_norm_act_backward(bg, bx, *bp, ec.EPS, True, [True] * 3)]
        torch.cuda.synchronize()
        runs.append(out)
    assert all(bool(torch.isfinite(t).all()) for t in runs[0])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_compile_fullgraph_forward_and_backward():
    torch._dynamo.reset()
    conv = ec.CONV_BY_NAME["3x3-c33-n126-3x5x7-s2"]
    g, x, w = _cdev(conv)
    b = ec.gaussian(9, (w.shape[0],)).to(DEV)
    bn = ec.NORM_BY_NAME["frozen_bn-2x3x5x7-relu"]
    gamma, beta, rm, rv = _bn_params(bn)
    # conv (33 -> 126, stride 2) -> instance norm + relu; and a frozen batch norm + relu on its own input
    gi = ec.gaussian(10, tuple(g.shape), ec.GRAD_SIGMA).to(DEV)
    gb, xb = bn.grad_out.to(DEV), bn.x.to(DEV)

    def loss(xx, ww, bb, xn, ga, be):
        y = torch.ops.oflow.instance_norm_act(torch.ops.oflow.conv2d_strided(xx, ww, bb, 2), ec.EPS, True)
        z = torch.ops.oflow.frozen_batch_norm_act(xn, ga, be, rm, rv, ec.EPS, True)
        return (y * gi).sum() + (z * gb).sum()

    grads = []
    for fn in (loss, torch.compile(loss, fullgraph=True, dynamic=False)):
        leaves = [t.clone().requires_grad_() for t in (x, w, b, xb, gamma, beta)]
        value = fn(*leaves)
        value.backward()
        grads.append((value.detach(),) + tuple(t.grad for t in leaves))
    torch.testing.assert_close(grads[1][0], grads[0][0], rtol=1e-5, atol=1e-9)
    assert all(torch.equal(a, b) for a, b in zip(grads[1][1:], grads[0][1:]))


# ----------------------------------------------------------------------------------------------------------
# encoders
# ----------------------------------------------------------------------------------------------------------
def _graph_nodes(root, needle: str) -> int:
    """The number of autograd nodes reachable from ``root`` whose class name contains ``needle``."""
    seen, stack, count = set(), [root], 0
    while stack:
        node = stack.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        count += needle in type(node).__name__.lower()
        stack.extend(fn for fn, _ in node.next_functions)
    return count


def _biases_under_instance_norm(model):
    """Names of the convolution biases whose output goes straight into a norm layer that subtracts a per-channel mean
    of its own input: an InstanceNorm2d without affine parameters, or a BatchNorm2d on batch statistics (train mode).
    Either removes a per-channel constant, so dL/dbias is exactly 0 and what autograd returns is rounding noise
    (tests/test_gpu_conv_backward.py::_biases_under_instance_norm). Found from the module structure."""
    plain = lambda n: ((isinstance(n, torch.nn.InstanceNorm2d) and not n.affine)  # noqa: E731
                       or (isinstance(n, torch.nn.BatchNorm2d) and n.training))
    names = set()
    for prefix, mod in model.named_modules():
        dot = prefix + "." if prefix else ""
        for conv, norm in (("conv1", "norm1"), ("conv2", "norm2")):
            c = getattr(mod, conv, None)
            if isinstance(c, torch.nn.Conv2d) and c.bias is not None and plain(getattr(mod, norm, None)):
                names.add(f"{dot}{conv}.bias")
        ds = getattr(mod, "downsample", None)
        if isinstance(ds, torch.nn.Sequential) and len(ds) == 2 and isinstance(ds[0], torch.nn.Conv2d) and plain(ds[1]):
            names.add(f"{dot}downsample.0.bias")
    return names


def _compare_grads(got, want, null, what):
    """Every gradient of ``got`` within a relative norm of 1e-3 of ``want``'s; for the exactly-zero ones (``null``) each
    side's norm within 1e-3 of the same convolution's weight-gradient norm."""
    assert set(got) == set(want)
    rels = {}
    for k, w in want.items():
        if k in null:
            wn = want[k[: -len("bias")] + "weight"].norm()
            rels[k] = max(float(got[k].norm() / wn), float(w.norm() / wn))
        else:
            assert float(w.norm()) > 0, k
            rels[k] = float((got[k] - w).norm() / w.norm())
    for k, rel in sorted(rels.items(), key=lambda t: -t[1])[:6]:
        print(f"{what}: {k}: {rel:.2e}" + (" (zero gradient: norm / weight-gradient norm)" if k in null else ""))
    bad = {k: r for k, r in rels.items() if not r <= 1e-3}
    assert not bad, (what, bad)


def _encoder(norm_fn: str, train_bn: bool = False):
    torch.manual_seed(11)
    enc = BasicEncoder(output_dim=64, norm_fn=norm_fn).to(DEV)
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for m in enc.modules():  # non-trivial statistics and affine parameters
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.running_mean.copy_(0.1 * torch.randn(n, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(n, generator=gen))
                m.weight.copy_(1 + 0.2 * torch.randn(n, generator=gen))
                m.bias.copy_(0.1 * torch.randn(n, generator=gen))
    enc.train()
    if norm_fn == "batch" and not train_bn:
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eval()
    return enc


def _encoder_run(enc, impl, x, gout):
    enc.encoder_backward_impl = impl
    enc.zero_grad(set_to_none=True)
    buffers = {k: v.clone() for k, v in enc.named_buffers()}
    out = enc(x)
    nodes = {n: _graph_nodes(out.grad_fn, n) for n in ("conv2d_strided", "norm_act", "convolution", "batchnorm")}
    out.backward(gout)
    with torch.no_grad():  # (train-mode batch norm updates its running statistics: put them back for the next run)
        for k, v in enc.named_buffers():
            v.copy_(buffers[k])
    return out.detach(), {k: p.grad.detach().clone() for k, p in enc.named_parameters()}, nodes


@pytest.mark.parametrize("norm_fn, train_bn", [("instance", False), ("batch", False), ("batch", True)],
                         ids=["instance", "batch-eval", "batch-train"])
def test_encoder_native_backward_matches_aten(norm_fn, train_bn):
    """``BasicEncoder`` on 2 x 3 x 40 x 56 with a fixed output gradient, "native" against "aten": equal outputs, every
    parameter gradient to a relative norm of 1e-3, 16 conv2d_strided nodes and 15 native norm nodes (none with batch
    norm in train mode: batch statistics stay the module, the convolutions stay native), no ATen convolution node, two
    native runs bit-identical. The biases in front of a norm that subtracts its own per-channel mean (instance norm,
    train-mode batch norm) have an exactly zero gradient and are held to 1e-3 of the weight-gradient norm instead.

    Runs under ``torch.backends.cudnn.flags(deterministic=True)``: at this size layer3's 128 -> 128 3x3 convolutions see
    2 x 128 x 5 x 7 inputs, for which MIOpen's default forward differs from call to call (measured: two runs of the
    unmodified "aten" encoder disagree by 3e-6, the module called twice on one input by 2.4e-7), so without the flag
    neither setting reproduces even itself. The flag restricts both settings' forward, the same ATen call, to MIOpen's
    deterministic solvers."""
    enc = _encoder(norm_fn, train_bn)
    x = ec.gaussian(21, (2, 3, 40, 56)).to(DEV)
    gout = ec.gaussian(22, (2, 64, 5, 7), ec.GRAD_SIGMA).to(DEV)
    with torch.backends.cudnn.flags(deterministic=True):
        out_a, grads_a, nodes_a = _encoder_run(enc, "aten", x, gout)
        out_n, grads_n, nodes_n = _encoder_run(enc, "native", x, gout)
        _dirty_allocator()
        out_n2, grads_n2, _ = _encoder_run(enc, "native", x, gout)
    assert nodes_a["conv2d_strided"] == 0 and nodes_a["norm_act"] == 0 and nodes_a["convolution"] == 16, nodes_a
    assert nodes_n["conv2d_strided"] == 16 and nodes_n["convolution"] == 0, nodes_n
    assert nodes_n["norm_act"] == (0 if train_bn else 15), nodes_n
    assert (nodes_n["batchnorm"] == 0) == (not train_bn), nodes_n
    assert torch.equal(out_n, out_a) and torch.equal(out_n2, out_n)
    null = _biases_under_instance_norm(enc)  # (also the biases in front of a batch norm on batch statistics)
    assert len(null) == (15 if norm_fn == "instance" or train_bn else 0)
    _compare_grads(grads_n, grads_a, null, f"encoder {norm_fn}" + (" (train-mode batch norm)" if train_bn else ""))
    assert all(torch.equal(grads_n[k], grads_n2[k]) for k in grads_n)
    assert all(bool(torch.isfinite(v).all()) for v in grads_n.values())


# ----------------------------------------------------------------------------------------------------------
# RAFT
# ----------------------------------------------------------------------------------------------------------
def _train_model():
    m = RAFT(iters=3)
    m.load_state_dict(synthetic.synthetic_state_dict(m.state_dict()))
    m = m.to(DEV).train()
    m.freeze_bn()
    return m


def test_training_step_with_native_encoder_backward():
    """One 128 x 128, 3-iteration training step with synthetic weights and batch norm frozen: (a) defaults, (b)
    ``encoder_backward_impl = "native"``, (c) both switches native. Equal losses; (b) and (c) match (a) on every
    parameter gradient to 1e-3; the graphs of (b) and (c) hold 32 conv2d_strided and 30 native norm nodes and (a) none;
    (c) holds no ATen convolution or batch-norm node; two runs of (c) give bit-identical gradients.

    Every setting runs under ``torch.backends.cudnn.flags(deterministic=True)``. The forward's convolutions are ATen's
    in all of them, and MIOpen's default forward solvers are not all reproducible (measured on the encoder test's
    2 x 128 x 5 x 7 layers). Without the flag the bit-identity assertion held in 100 steps run for the purpose and in
    five of six whole-suite runs; in the sixth every listed gradient of the second (c) run differed, with equal losses.
    The flag takes out the one source of run-to-run differences that is known; that it was the cause of that one
    failure is a supposition."""
    img0, img1 = (x.to(DEV) for x in synthetic.synthetic_pair(1, 128, 128, seed=5))
    target = torch.from_numpy(synthetic.hash_normal(31, (1, 2, 128, 128), 2.0)).to(DEV)
    valid = (torch.from_numpy(synthetic.hash_normal(32, (1, 128, 128), 1.0)) > -1.0).float().to(DEV)
    settings = {"a": ("aten", "aten"), "b": ("native", "aten"), "c": ("native", "native"), "c2": ("native", "native")}
    grads, losses, nodes = {}, {}, {}
    for tag, (enc_impl, conv_impl) in settings.items():
        model = _train_model()
        assert model.encoder_backward_impl == "aten" and model.conv_backward_impl == "aten"  # the defaults
        model.encoder_backward_impl, model.conv_backward_impl = enc_impl, conv_impl
        if tag == "c2":
            _dirty_allocator()
        with torch.backends.cudnn.flags(deterministic=True):  # (the forward's convolutions: see the docstring)
            loss = model.training_step((img0, img1, target, valid), 0)
            nodes[tag] = {n: _graph_nodes(loss.grad_fn, n)
                          for n in ("conv2d_strided", "norm_act", "conv2d_same", "convolution", "batchnorm")}
            loss.backward()
        losses[tag] = loss.detach()
        grads[tag] = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    print("graph nodes:", nodes)
    assert nodes["a"]["conv2d_strided"] == 0 and nodes["a"]["norm_act"] == 0 and nodes["a"]["conv2d_same"] == 0
    for tag in ("b", "c"):
        assert nodes[tag]["conv2d_strided"] == 32 and nodes[tag]["norm_act"] == 30, nodes[tag]
    assert nodes["b"]["conv2d_same"] == 0 and nodes["c"]["conv2d_same"] == 45
    assert nodes["b"]["convolution"] == 45 and nodes["b"]["batchnorm"] == 0
    assert nodes["c"]["convolution"] == 0 and nodes["c"]["batchnorm"] == 0
    assert all(torch.equal(losses[t], losses["a"]) for t in settings)
    null = _biases_under_instance_norm(model)
    assert len(null) == 15 and all(k.startswith("fnet.") for k in null)
    _compare_grads(grads["b"], grads["a"], null, "training step (b)")
    _compare_grads(grads["c"], grads["a"], null, "training step (c)")
    differ = [k for k in grads["c"] if not torch.equal(grads["c"][k], grads["c2"][k])]
    assert not differ, differ
    model.encoder_backward_impl = "miopen"
    with pytest.raises(ValueError, match="encoder_backward_impl"):
        model.training_step((img0, img1, target, valid), 0)
