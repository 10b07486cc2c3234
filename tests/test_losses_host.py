"""The unsupervised losses without a GPU: the CPU path of optical_flow.losses against the float64 reference
(tests/losses_cases.py), the calibration of the tolerances, gradcheck, the closed-form gradients against float64
autograd, the exact-zero cases, every validation error, the operators' registration / schemas / Meta kernels, the C
ABI's argument errors (nothing is launched) and unsupervised_sequence_loss on CPU tensors."""
import os

import numpy as np
import pytest
import torch

import losses_cases as lc
import optical_flow
from conftest import GOLDEN
from optical_flow import _native, _ops, census_loss, smoothness_loss

ZERO_CENSUS = [n for n in lc.CENSUS_IDS if n.startswith("1x3x6x20-") or n.endswith("-zero")]
ZERO_SMOOTH = ["1x1x1x1-o1-gauss-smooth", "1x1x1x1-o2-gauss-smooth", "2x3x2x2-o2-gauss-smooth"]


def _census_cpu(case, dtype=torch.float32):
    f0, f1, mask = lc.census_tensors(case, requires_grad=True, dtype=dtype)
    loss, s_map = census_loss(f0, f1, mask, case.patch, case.image_range, return_map=True)
    grads = torch.autograd.grad(loss * lc.GRAD_LOSS, [f0, f1])
    return loss, grads, s_map


def _smooth_cpu(case, dtype=torch.float32):
    flow, image = lc.smooth_tensors(case, requires_grad=True, dtype=dtype)
    loss = smoothness_loss(flow, image, case.order, case.edge_weight, case.image_range)
    (grad,) = torch.autograd.grad(loss * lc.GRAD_LOSS, [flow])
    return loss, grad


# ------------------------------------------------------------------------------------------ CPU path and calibration
@pytest.mark.parametrize("name", lc.CENSUS_IDS)
def test_census_cpu_path_meets_the_reference(name):
    case = lc.CENSUS_BY_NAME[name]
    loss, grads, s_map = _census_cpu(case)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and not s_map.requires_grad
    assert tuple(s_map.shape) == (case.frame0.shape[0], 1) + case.frame0.shape[2:] and s_map.dtype == torch.float32
    lc.assert_census(case, "cpu", loss, grads, s_map)


@pytest.mark.parametrize("name", lc.SMOOTH_IDS)
def test_smoothness_cpu_path_meets_the_reference(name):
    case = lc.SMOOTH_BY_NAME[name]
    loss, grad = _smooth_cpu(case)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    lc.assert_smooth(case, "cpu", loss, grad)


def test_calibration_the_fp32_composition_stays_within_a_quarter_of_every_k():
    worst = {"census_loss": 0.0, "census_grad": 0.0, "census_map": 0.0, "smooth_loss": 0.0, "smooth_grad": 0.0}
    for case in lc.CENSUS_CASES:
        f0, f1, mask = lc.census_tensors(case, requires_grad=True)
        loss, s_map = lc.census_compose(f0, f1, mask, case.patch, case.image_range)
        grads = torch.autograd.grad(loss * lc.GRAD_LOSS, [f0, f1])
        for key, value in lc.census_ratios(case, loss, grads, s_map).items():
            worst["census_" + key] = max(worst["census_" + key], value)
    for case in lc.SMOOTH_CASES:
        flow, image = lc.smooth_tensors(case, requires_grad=True)
        loss = lc.smooth_compose(flow, image, case.order, case.edge_weight, case.image_range)
        (grad,) = torch.autograd.grad(loss * lc.GRAD_LOSS, [flow])
        for key, value in lc.smooth_ratios(case, loss, grad).items():
            worst["smooth_" + key] = max(worst["smooth_" + key], value)
    print("measured:", {k: round(v, 3) for k, v in worst.items()}, "recorded:", lc.MEASURED)
    ks = {"census_loss": lc.K_CENSUS_LOSS, "census_grad": lc.K_CENSUS_GRAD, "census_map": lc.K_CENSUS_MAP,
          "smooth_loss": lc.K_SMOOTH_LOSS, "smooth_grad": lc.K_SMOOTH_GRAD}
    assert set(lc.MEASURED) == set(ks)
    for key, k in ks.items():
        assert worst[key] <= k / 4, (key, worst[key], k)
        assert lc.MEASURED[key] <= k / 4 and k / 4 <= 1.3 * lc.MEASURED[key] + 0.5, (key, "K is not 4 x the rounded maximum")


def test_the_tolerance_checks_refuse_non_finite_values():
    """A NaN or inf in anything that is checked counts as an infinite error, and is named."""
    case = lc.CENSUS_BY_NAME["2x3x23x133-p7-near-float"]
    ref = lc.census_reference(case)
    good = [torch.from_numpy(g).float() for g in ref.grads]
    loss, s_map = torch.tensor(ref.loss, dtype=torch.float32), torch.from_numpy(ref.s).float()
    lc.assert_census(case, "reference", loss, good, s_map)
    for bad in (float("nan"), float("inf")):
        broken = [good[0].clone(), good[1].clone()]
        broken[1][1, 2, 10, 70] = bad
        poked = s_map.clone()
        poked[0, 0, 10, 70] = bad
        assert lc.census_ratios(case, torch.tensor(bad), broken, poked) == {"loss": float("inf"), "grad": float("inf"),
                                                                            "map": float("inf")}
        for kw in (dict(loss=torch.tensor(bad)), dict(grads=broken), dict(grads=[None, broken[1]]), dict(s_map=poked)):
            with pytest.raises(AssertionError, match="non-finite"):
                lc.assert_census(case, "broken", **kw)
    case = lc.SMOOTH_BY_NAME["2x3x5x65-o2-gauss-smooth"]
    ref = lc.smooth_reference(case)
    loss, grad = torch.tensor(ref.loss, dtype=torch.float32), torch.from_numpy(ref.grad).float()
    lc.assert_smooth(case, "reference", loss, grad)
    for bad in (float("nan"), float("-inf")):
        broken = grad.clone()
        broken[1, 0, 2, 64] = bad
        assert lc.smooth_ratios(case, torch.tensor(bad), broken) == {"loss": float("inf"), "grad": float("inf")}
        for kw in (dict(loss=torch.tensor(bad)), dict(grad=broken)):
            with pytest.raises(AssertionError, match="non-finite"):
                lc.assert_smooth(case, "broken", **kw)


# ------------------------------------------------------------------------------------------ gradients
def test_gradcheck_of_the_cpu_path_in_float64():
    for name in ("1x1x7x7-p7-near-float", "1x3x9x70-p3-near-float"):  # the two smallest non-degenerate census cases
        case = lc.CENSUS_BY_NAME[name]
        f0, f1, mask = lc.census_tensors(case, requires_grad=True, dtype=torch.float64)
        if name.startswith("1x3x9x70"):  # (a strip of it: gradcheck perturbs every element)
            f0, f1, mask = (t[..., :12].detach().clone() for t in (f0, f1, mask))
            f0.requires_grad_(), f1.requires_grad_()
        if name.startswith("1x1x7x7"):
            mask = torch.ones_like(mask)
        fn = lambda a, b: census_loss(a, b, mask, case.patch, case.image_range)  # noqa: E731
        assert census_loss(f0, f1, mask, case.patch, case.image_range).dtype == torch.float64
        assert torch.autograd.gradcheck(fn, (f0, f1), eps=1e-4, atol=1e-7, rtol=1e-5)
    for name in ("1x3x1x9-o1-gauss-smooth", "2x3x5x64-o2-gauss-smooth"):
        case = lc.SMOOTH_BY_NAME[name]
        flow, image = lc.smooth_tensors(case, requires_grad=True, dtype=torch.float64)
        flow, image = flow[..., :9].detach().clone().requires_grad_(), image[..., :9].clone()
        fn = lambda f: smoothness_loss(f, image, case.order, case.edge_weight, case.image_range)  # noqa: E731
        assert torch.autograd.gradcheck(fn, (flow,), eps=1e-5, atol=1e-8, rtol=1e-5)


@pytest.mark.parametrize("name", lc.CENSUS_IDS)
def test_census_closed_form_gradients_equal_float64_autograd(name):
    """(1e-7 of the bound: the float64 composition forms t_0 - t_1 without the cancellation, the reference with it, and
    at |delta| ~ 250 the plain form loses 1e5 x 2^-53 of the term.)"""
    case = lc.CENSUS_BY_NAME[name]
    ref = lc.census_reference(case)
    loss, grads, s_map = _census_cpu(case, torch.float64)
    assert loss.dtype == torch.float64 and abs(float(loss.detach()) - ref.loss) <= 1e-12 * ref.loss
    for got, want, bound in zip(grads, ref.grads, ref.bounds):
        assert (np.abs(got.numpy() - want) <= 1e-7 * bound).all()


@pytest.mark.parametrize("name", lc.SMOOTH_IDS)
def test_smoothness_closed_form_gradients_equal_float64_autograd(name):
    case = lc.SMOOTH_BY_NAME[name]
    ref = lc.smooth_reference(case)
    loss, grad = _smooth_cpu(case, torch.float64)
    # (the reference divides the fp32 edge weight by the fp32 range as the kernel's arguments arrive; exp turns the
    # quotient's 2^-24 into up to 50 x 2^-24 on the noise images)
    assert loss.dtype == torch.float64 and abs(float(loss.detach()) - ref.loss) <= 1e-5 * ref.loss
    assert (np.abs(grad.numpy() - ref.grad) <= 1e-5 * ref.bound).all()


# ------------------------------------------------------------------------------------------ the exact zeros
@pytest.mark.parametrize("name", ZERO_CENSUS)
def test_census_exact_zero_cases(name):
    case = lc.CENSUS_BY_NAME[name]
    ref = lc.census_reference(case)
    assert ref.loss == 0.0 and not ref.grads[0].any() and not ref.grads[1].any()
    loss, grads, s_map = _census_cpu(case)
    assert float(loss) == 0.0 and not grads[0].any() and not grads[1].any()
    if name.startswith("1x3x6x20-"):
        assert not s_map.any()


def test_census_identical_and_constant_frames():
    for kind in ("identical", "constant"):
        case = lc.CENSUS_BY_NAME[f"2x3x23x133-p7-{kind}-none"]
        loss, grads, s_map = _census_cpu(case)
        assert abs(float(loss) - 0.01**0.4) <= lc.K_CENSUS_LOSS * lc.U * 0.01**0.4
        assert not grads[0].any() and not grads[1].any() and not s_map.any()


@pytest.mark.parametrize("name", ZERO_SMOOTH)
def test_smoothness_empty_domains_give_exactly_zero(name):
    case = lc.SMOOTH_BY_NAME[name]
    assert lc.smooth_reference(case).loss == 0.0
    loss, grad = _smooth_cpu(case)
    assert float(loss) == 0.0 and not grad.any()


def test_smoothness_of_a_constant_flow():
    for order in (1, 2):
        case = lc.SMOOTH_BY_NAME[f"2x3x33x130-o{order}-const-smooth"]
        loss, grad = _smooth_cpu(case)
        assert float(loss) > 0 and not grad.any()  # sqrt(0 + 0.001^2) per element, no slope at 0
    one_direction = lc.SMOOTH_BY_NAME["1x3x1x9-o1-gauss-smooth"]
    assert lc.smooth_reference(one_direction).loss > 0


# ------------------------------------------------------------------------------------------ validation
def test_census_validation_errors():
    f, m = torch.zeros(2, 3, 9, 9), torch.ones(2, 1, 9, 9)
    with pytest.raises(TypeError, match="census_loss: frame0 must be a torch.Tensor"):
        census_loss(f.numpy(), f)
    with pytest.raises(TypeError, match="census_loss: frame1 must be a torch.Tensor"):
        census_loss(f, None)
    with pytest.raises(TypeError, match="census_loss: mask must be a torch.Tensor"):
        census_loss(f, f, m.numpy())
    with pytest.raises(TypeError, match="census_loss: frame0 must be a floating-point tensor"):
        census_loss(f.long(), f)
    with pytest.raises(TypeError, match="census_loss: mask must be a floating-point or bool tensor"):
        census_loss(f, f, m.long())
    with pytest.raises(ValueError, match=r"census_loss: frame0 .* must be equal \(B, C, H, W\)"):
        census_loss(f[0], f[0])
    with pytest.raises(ValueError, match=r"census_loss: frame0 .* and frame1 .* must be equal"):
        census_loss(f, f[..., :-1])
    with pytest.raises(ValueError, match=r"census_loss: mask must be \(B, 1, H, W\)"):
        census_loss(f, f, m[:, :, :-1])
    with pytest.raises(ValueError, match="census_loss: all tensors must be on one device"):
        census_loss(f, f.to("meta"))
    with pytest.raises(ValueError, match="census_loss: all tensors must be on one device"):
        census_loss(f, f, m.to("meta"))
    for patch in (1, 4, 9):
        with pytest.raises(ValueError, match="census_loss: patch must be one of"):
            census_loss(f, f, patch=patch)
    for patch in (7.0, 7.5, True, "7"):
        with pytest.raises(TypeError, match="census_loss: patch must be an int"):
            census_loss(f, f, patch=patch)
    for bad in (0.0, -255.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="census_loss: image_range"):
            census_loss(f, f, image_range=bad)
    assert census_loss(f, f, m > 0).dtype == torch.float32  # a bool mask is accepted
    assert optical_flow.losses.census_loss is census_loss and optical_flow.losses.smoothness_loss is smoothness_loss
    assert "census_loss" in optical_flow.__all__ and "smoothness_loss" in optical_flow.__all__
    for fn in (census_loss, smoothness_loss):
        assert "published" in fn.__doc__ and "tuned" in fn.__doc__


def test_smoothness_validation_errors():
    fl, im = torch.zeros(2, 2, 5, 6), torch.zeros(2, 3, 5, 6)
    with pytest.raises(TypeError, match="smoothness_loss: flow must be a torch.Tensor"):
        smoothness_loss(None, im)
    with pytest.raises(TypeError, match="smoothness_loss: image must be a torch.Tensor"):
        smoothness_loss(fl, im.numpy())
    with pytest.raises(TypeError, match="smoothness_loss: image must be a floating-point tensor"):
        smoothness_loss(fl, im.byte())
    with pytest.raises(ValueError, match=r"smoothness_loss: image must be \(B, C, H, W\)"):
        smoothness_loss(fl, im[0])
    with pytest.raises(ValueError, match=r"smoothness_loss: flow must be \(B, 2, H, W\)"):
        smoothness_loss(im, im)
    with pytest.raises(ValueError, match=r"smoothness_loss: flow must be \(B, 2, H, W\)"):
        smoothness_loss(fl[..., :-1], im)
    with pytest.raises(ValueError, match="smoothness_loss: all tensors must be on one device"):
        smoothness_loss(fl, im.to("meta"))
    for order in (0, 3):
        with pytest.raises(ValueError, match="smoothness_loss: order must be one of"):
            smoothness_loss(fl, im, order=order)
    for order in (1.0, 1.5, True):
        with pytest.raises(TypeError, match="smoothness_loss: order must be an int"):
            smoothness_loss(fl, im, order=order)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="smoothness_loss: image_range"):
            smoothness_loss(fl, im, image_range=bad)
    for bad in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(ValueError, match="smoothness_loss: edge_weight must be a finite number"):
            smoothness_loss(fl, im, edge_weight=bad)
    im.requires_grad_()
    fl.requires_grad_()
    smoothness_loss(fl, im).backward()
    assert im.grad is None and fl.grad is not None  # the image is data


# ------------------------------------------------------------------------------------------ the registered operators
def test_ops_are_registered_with_the_recorded_schemas():
    _native.load()
    assert _ops.OPS_LOSSES == ("census_loss", "census_loss_backward", "smoothness_loss", "smoothness_loss_backward")
    assert not set(_ops.OPS_LOSSES) & (set(_ops.OPS) | set(_ops.OPS_SPLAT))
    with open(os.path.join(GOLDEN, "op_schemas_losses.txt")) as f:
        recorded = [line.rstrip("\n") for line in f if line.strip()]
    assert [str(getattr(torch.ops.oflow, name).default._schema) for name in _ops.OPS_LOSSES] == recorded
    for name in _ops.OPS_LOSSES:
        for key in ("CUDA", "CPU", "Meta"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"oflow::{name}", key), (name, key)
    for sym in ("oflow_census_loss_workspace_bytes", "oflow_census_loss_f32", "oflow_census_loss_backward_f32",
                "oflow_smoothness_loss_workspace_bytes", "oflow_smoothness_loss_f32", "oflow_smoothness_loss_backward_f32"):
        assert sym in _native.SYMBOLS


def test_meta_kernels_and_gradients_on_meta_tensors():
    _native.load()
    meta = lambda *s, **k: torch.empty(*s, device="meta", **k)  # noqa: E731
    f0, f1, mask = meta(3, 3, 55, 128), meta(3, 3, 55, 128, dtype=torch.float64), meta(3, 1, 55, 128, dtype=torch.bool)
    for m in (None, mask, meta(3, 1, 55, 128)):
        loss, sum_m, s_map = torch.ops.oflow.census_loss(f0, f1, m, 7, 255.0)
        assert tuple(loss.shape) == () and loss.dtype == torch.float32 and loss.device.type == "meta"
        assert tuple(sum_m.shape) == () and sum_m.dtype == torch.float64
        assert tuple(s_map.shape) == (3, 1, 55, 128) and s_map.dtype == torch.float32
        for om in ([True, True], [True, False], [False, True]):
            gs = torch.ops.oflow.census_loss_backward(loss, f0, f1, m, sum_m, s_map, 7, 255.0, om)
            assert [tuple(g.shape) for g in gs] == [(3, 3, 55, 128) if o else (0,) for o in om]
            assert all(g.dtype == torch.float32 for g in gs)
    with pytest.raises(RuntimeError, match=r"must be equal \(B, C, H, W\)"):
        torch.ops.oflow.census_loss(f0, meta(3, 3, 55, 64), None, 7, 255.0)
    with pytest.raises(RuntimeError, match=r"mask must be \(B, 1, H, W\)"):
        torch.ops.oflow.census_loss(f0, f1, meta(3, 2, 55, 128), 7, 255.0)
    with pytest.raises(RuntimeError, match="not one of 3, 5, 7"):
        torch.ops.oflow.census_loss(f0, f1, None, 4, 255.0)
    with pytest.raises(RuntimeError, match="image_range"):
        torch.ops.oflow.census_loss(f0, f1, None, 7, 0.0)
    flow, image = meta(3, 2, 55, 128), meta(3, 3, 55, 128)
    for order in (1, 2):
        loss = torch.ops.oflow.smoothness_loss(flow, image, order, 150.0, 255.0)
        assert tuple(loss.shape) == () and loss.dtype == torch.float32
        g = torch.ops.oflow.smoothness_loss_backward(loss, flow, image, order, 150.0, 255.0)
        assert tuple(g.shape) == (3, 2, 55, 128) and g.dtype == torch.float32
    with pytest.raises(RuntimeError, match=r"flow must be \(B, 2, H, W\)"):
        torch.ops.oflow.smoothness_loss(image, image, 1, 150.0, 255.0)
    with pytest.raises(RuntimeError, match="not 1 or 2"):
        torch.ops.oflow.smoothness_loss(flow, image, 3, 150.0, 255.0)
    # gradients flow on meta tensors: the autograd formulas are wired, sum M and the map are not differentiable
    a, b = f0.clone().requires_grad_(), f0.clone().requires_grad_()
    loss, sum_m, s_map = torch.ops.oflow.census_loss(a, b, mask, 5, 255.0)
    assert loss.requires_grad and not sum_m.requires_grad and not s_map.requires_grad
    ga, gb = torch.autograd.grad(loss, [a, b])
    assert tuple(ga.shape) == tuple(gb.shape) == (3, 3, 55, 128)
    loss, _, _ = torch.ops.oflow.census_loss(f0, b, None, 3, 255.0)  # only frame1 needs one
    (gb,) = torch.autograd.grad(loss, [b])
    assert tuple(gb.shape) == (3, 3, 55, 128)
    fl = flow.clone().requires_grad_()
    (g,) = torch.autograd.grad(torch.ops.oflow.smoothness_loss(fl, image, 2, 150.0, 255.0), [fl])
    assert tuple(g.shape) == (3, 2, 55, 128)


def test_cpu_tensors_reaching_the_raw_ops_raise():
    _native.load()
    f, m, fl = torch.zeros(1, 3, 9, 9), torch.ones(1, 1, 9, 9), torch.zeros(1, 2, 9, 9)
    one, one64 = torch.ones(()), torch.ones((), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.oflow.census_loss(f, f, None, 7, 255.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.oflow.census_loss_backward(one, f, f, m, one64, m, 7, 255.0, [True, True])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.oflow.smoothness_loss(fl, f, 1, 150.0, 255.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.oflow.smoothness_loss_backward(one, fl, f, 1, 150.0, 255.0)


# ------------------------------------------------------------------------------------------ the C ABI's argument errors
def test_c_abi_argument_errors_without_launch():
    lib = _native.load()
    NULL, SHAPE, MODE, ALIGN = -1, -2, -6, -7
    A = 1 << 20
    f0, f1, mk, sm, ws, lo, su, gl, g0, g1 = (A * k for k in range(1, 11))
    size, fwd, bwd = lib.oflow_census_loss_workspace_bytes, lib.oflow_census_loss_f32, lib.oflow_census_loss_backward_f32
    assert size(1, 7, 7) == 16 and size(2, 23, 133) == 16 * 2 * 3 * 3 and size(8, 436, 1024) == 16 * 8 * 55 * 16
    for b, h, w in ((0, 9, 9), (1, 0, 9), (1, 9, 0), (65536, 9, 9), (1, 16384, 16385)):
        assert size(b, h, w) == 0
        assert fwd(f0, f1, None, 0, b, 3, h, w, 7, 255.0, sm, ws, lo, su, None) == SHAPE
        assert bwd(gl, f0, f1, None, 0, sm, su, b, 3, h, w, 7, 255.0, g0, g1, None) == SHAPE
    assert fwd(f0, f1, None, 0, 1, 0, 9, 9, 7, 255.0, sm, ws, lo, su, None) == SHAPE  # C
    assert fwd(f0, f1, None, 0, 1, 3, 9, 9, 7, 0.0, sm, ws, lo, su, None) == SHAPE  # image_range
    for miss in (0, 1, 11, 12, 13):  # frame0, frame1, workspace, loss, sum_m
        args = [f0, f1, None, 0, 1, 3, 9, 9, 7, 255.0, sm, ws, lo, su, None]
        args[miss] = None
        assert fwd(*args) == NULL
    assert fwd(f0, f1, None, 1, 1, 3, 9, 9, 7, 255.0, sm, ws, lo, su, None) == NULL  # a mask kind without a mask
    assert fwd(f0, f1, mk, 3, 1, 3, 9, 9, 7, 255.0, sm, ws, lo, su, None) == MODE
    for patch in (1, 4, 9):
        assert fwd(f0, f1, None, 0, 1, 3, 9, 9, patch, 255.0, sm, ws, lo, su, None) == MODE
    assert fwd(f0 + 2, f1, None, 0, 1, 3, 9, 9, 7, 255.0, sm, ws, lo, su, None) == ALIGN
    assert fwd(f0, f1, None, 0, 1, 3, 9, 9, 7, 255.0, sm, ws + 4, lo, su, None) == ALIGN
    assert fwd(f0, f1, None, 0, 1, 3, 9, 9, 7, 255.0, sm, ws, lo, su + 4, None) == ALIGN
    assert bwd(None, f0, f1, None, 0, sm, su, 1, 3, 9, 9, 7, 255.0, g0, g1, None) == NULL
    assert bwd(gl, f0, f1, None, 0, sm, None, 1, 3, 9, 9, 7, 255.0, g0, g1, None) == NULL
    assert bwd(gl, f0, f1, None, 0, sm, su, 1, 3, 9, 9, 7, 255.0, None, None, None) == NULL  # nothing asked for
    assert bwd(gl, f0, f1, None, 0, sm, su, 1, 3, 9, 9, 6, 255.0, g0, g1, None) == MODE
    assert bwd(gl, f0, f1, None, 0, sm, su, 1, 3, 9, 9, 7, 255.0, g0, g1 + 1, None) == ALIGN
    # smoothness
    fl, im, gf = f0, f1, g0
    size, fwd, bwd = (lib.oflow_smoothness_loss_workspace_bytes, lib.oflow_smoothness_loss_f32,
                      lib.oflow_smoothness_loss_backward_f32)
    assert size(1, 1, 1) == 16 and size(2, 33, 130) == 16 * ((2 * 33 * 130 + 255) // 256)
    for b, h, w in ((0, 9, 9), (1, 0, 9), (1, 9, 0), (65536, 9, 9), (1, 16384, 16385)):
        assert size(b, h, w) == 0
        assert fwd(fl, im, b, 3, h, w, 1, 150.0, 255.0, ws, lo, None) == SHAPE
        assert bwd(gl, fl, im, b, 3, h, w, 1, 150.0, 255.0, gf, None) == SHAPE
    assert fwd(fl, im, 1, 3, 9, 9, 1, 150.0, 0.0, ws, lo, None) == SHAPE
    for miss in (0, 1, 9, 10):
        args = [fl, im, 1, 3, 9, 9, 1, 150.0, 255.0, ws, lo, None]
        args[miss] = None
        assert fwd(*args) == NULL
    for order in (0, 3):
        assert fwd(fl, im, 1, 3, 9, 9, order, 150.0, 255.0, ws, lo, None) == MODE
        assert bwd(gl, fl, im, 1, 3, 9, 9, order, 150.0, 255.0, gf, None) == MODE
    assert fwd(fl, im, 1, 3, 9, 9, 1, 150.0, 255.0, ws + 4, lo, None) == ALIGN
    assert bwd(None, fl, im, 1, 3, 9, 9, 1, 150.0, 255.0, gf, None) == NULL
    assert bwd(gl, fl, im, 1, 3, 9, 9, 1, 150.0, 255.0, None, None) == NULL
    assert bwd(gl, fl, im, 1, 3, 9, 9, 1, 150.0, 255.0, gf + 2, None) == ALIGN


# ------------------------------------------------------------------------------------------ the training entry point
def test_unsupervised_sequence_loss_on_cpu_equals_the_sum_written_out():
    import torch.nn.functional as F

    import model
    from model.raft import unsupervised_sequence_loss
    from optical_flow import normalize, warp_grid

    assert model.unsupervised_sequence_loss is unsupervised_sequence_loss and "unsupervised_sequence_loss" in model.__all__
    g = torch.Generator().manual_seed(11)
    img0 = torch.randint(0, 256, (2, 3, 23, 40), generator=g).float()
    img1 = (img0 + 6 * torch.randn((2, 3, 23, 40), generator=g)).clamp(0, 255)
    preds = [torch.randn((2, 2, 23, 40), generator=g).requires_grad_() for _ in range(3)]
    mask = torch.rand((2, 1, 23, 40), generator=g) < 0.8
    gamma, wc, ws, order = 0.7, 0.5, 2.0, 2
    got = unsupervised_sequence_loss(preds, img0, img1, mask, gamma=gamma, w_census=wc, w_smooth=ws, smooth_order=order)
    want = 0.0
    for i, flow in enumerate(preds):
        grid = warp_grid(normalize(flow).permute(0, 2, 3, 1))
        warped = F.grid_sample(img1, grid, mode="bilinear", padding_mode="border", align_corners=True)
        want = want + gamma ** (2 - i) * (wc * census_loss(img0, warped, mask) + ws * smoothness_loss(flow, img0, order=order))
    assert got.dim() == 0 and float(got) == float(want)
    got.backward()
    assert all(p.grad is not None and p.grad.abs().sum() > 0 for p in preds)
    # zero flow with align_corners=True: the warp is the identity, so the census term sees identical frames
    zero = [torch.zeros(2, 2, 23, 40)]
    same = unsupervised_sequence_loss(zero, img0, img0, w_smooth=0.0)
    assert abs(float(same) - 0.01**0.4) <= 1e-6
    doc = unsupervised_sequence_loss.__doc__
    assert "align_corners=True" in doc and "Q8" in doc and "untuned" in doc
    assert "untuned" in model.RAFT.unsupervised_step.__doc__
